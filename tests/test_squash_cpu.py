"""Squash clustering of a cohort's samples, no device: the rule of include/epik_amd.h restated here in numpy against
epik_amd_cohort_squash_host -- all 32 bytes of every record --, forged cohorts for the tie rule and the edges, a case
derived by hand, properties on random cohorts, the C ABI's refusals, the drivers' and the launcher's flag, the two files
and the stand-alone host binary (plain and under ASan + UBSan).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, numpy_kr, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NONE = 0xFFFFFFFF


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def numpy_planes(mass, first):
    """C_s[b], B_s[b] and T_s of the KR rule, as numpy_kr forms them."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    first = np.asarray(first, dtype=np.int64)
    prefix = np.zeros((s, n + 1), dtype=U64)
    np.cumsum(mass, axis=1, dtype=U64, out=prefix[:, 1:])
    total = prefix[:, n]
    clade = prefix[:, 1:] - prefix[:, first]
    below = clade - mass
    with np.errstate(invalid="ignore", divide="ignore"):
        c = clade.astype(np.float64) / total.astype(np.float64)[:, None]
        b = below.astype(np.float64) / total.astype(np.float64)[:, None]
    return c, b, total


def sequential_kr(cx, bx, c, b, half):
    """KR(x, y) for every row y of (c, b): the terms as arrays, then np.add.accumulate along the branches, which adds
    one element after the other in ascending order -- the rule's acc = acc + term (acc = +0.0 + term[0] is term[0],
    every term being >= +0.0).  test_the_restatement_s_sum_is_numpy_kr_s ties it to numpy_kr's python loop."""
    with np.errstate(invalid="ignore"):
        terms = half[None, :] * (np.abs(cx[None, :] - c) + np.abs(bx[None, :] - b))
    return np.add.accumulate(terms, axis=1)[:, -1]


def numpy_squash(mass, first, branch_length):
    """(records [S - 1], num_merges) by the header's text, slot by slot."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    half = 0.5 * np.asarray(branch_length, dtype=np.float64)
    c, b, total = numpy_planes(mass, first)
    live = total > 0
    w = np.ones(s, dtype=np.int64)
    node = np.arange(s, dtype=np.int64)
    d = numpy_kr(mass, first, branch_length)                      # D[r][c] = KR(r, c): the matrix epik_amd_cohort_kr gives
    records = np.zeros(max(s - 1, 0), dtype=capi.SQUASH_MERGE)
    records["a"] = records["b"] = NONE
    upper = np.triu(np.ones((s, s), dtype=bool), 1)
    t = 0
    while live.sum() >= 2:
        scan = np.where(upper & live[:, None] & live[None, :], d, np.inf)
        r, col = divmod(int(np.argmin(scan)), s)                  # (the first of the smallest, in row-major order)
        big = np.float64(w[r] + w[col])
        cm = (np.float64(w[r]) * c[r] + np.float64(w[col]) * c[col]) / big
        bm = (np.float64(w[r]) * b[r] + np.float64(w[col]) * b[col]) / big
        lengths = sequential_kr(cm, bm, c[[r, col]], b[[r, col]], half)   # (the planes of r and c as they were)
        records[t] = (node[r], node[col], d[r, col], lengths[0], lengths[1])
        c[r], b[r] = cm, bm
        w[r] += w[col]
        node[r] = s + t
        live[col] = False
        others = np.flatnonzero(live & (np.arange(s) != r))
        if len(others):
            d[r, others] = d[others, r] = sequential_kr(cm, bm, c[others], b[others], half)
        t += 1
    return records, t


def assert_records(got, want, what=""):
    """Every byte of every record."""
    want_records, count = want
    assert len(got) == count, (what, len(got), count)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(want_records[:count])
    assert a.dtype == capi.SQUASH_MERGE and a.tobytes() == b.tobytes(), (what, a, b)


def host_all_records(mass, first, bl):
    """All S - 1 records and the count, straight from the C entry (squash_host of the package checks and drops the
    unused ones)."""
    lib = capi.load()
    mass = np.ascontiguousarray(mass, dtype=U64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    bl = np.ascontiguousarray(bl, dtype=np.float64)
    s, n = mass.shape
    records = np.zeros(max(s - 1, 1), dtype=capi.SQUASH_MERGE)
    records.view(np.uint8)[:] = 0xA5
    count = ctypes.c_uint32(12345)
    assert lib.epik_amd_cohort_squash_host(mass.ctypes.data, s, n, first.ctypes.data, bl.ctypes.data, records.ctypes.data,
                                           ctypes.byref(count)) == capi.OK
    return records[:s - 1], count.value


def test_the_restatement_s_sum_is_numpy_kr_s():
    parent, bl = tree_case("tree2999")
    first = numpy_first(parent)
    mass = random_cells(np.random.default_rng(77), 5, len(parent))
    c, b, _ = numpy_planes(mass, first)
    want = numpy_kr(mass, first, bl)
    for x in range(5):
        got = sequential_kr(c[x], b[x], c, b, 0.5 * bl)
        got[x] = 0.0
        assert same_bits(got, want[x])


@pytest.mark.parametrize("tree_name,num_samples", [(t, s) for t in ("one", "tree15", "tree2999") for s in (1, 2, 3, 33)] +
                         [("ladder10399", 3)])
def test_squash_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    parent, bl = tree_case(tree_name)
    first = numpy_first(parent)
    rng = np.random.default_rng(2000 + num_samples)
    mass = random_cells(rng, num_samples, len(parent), empty=1)
    want, count = numpy_squash(mass, first, bl)
    records, got_count = host_all_records(mass, first, bl)
    assert got_count == count == max(0, int((mass.sum(axis=1, dtype=U64) > 0).sum()) - 1)
    assert records.tobytes() == want.tobytes(), (records, want)
    assert_records(cohort_mod.squash_host(mass, first, bl), (want, count))


# ---- forged cohorts: the tie rule and the edges ------------------------------------------------------------------------
BALANCED = np.array([2, 2, 6, 5, 5, 6, -1])                       # ((0,1)2,(3,4)5)6


def forged_cohorts():
    """name -> (mass, first, branch_length)"""
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    n = len(parent)
    rng = np.random.default_rng(42)
    x, y, z = (random_cells(rng, 1, n)[0] for _ in range(3))
    zero = np.zeros(n, U64)
    sym_first = numpy_first(BALANCED)
    sym_bl = np.array([0.5, 0.25, 0.125, 0.5, 0.25, 0.125, 0.0])  # the two cherries alike
    leaf = lambda b, m=1: np.eye(7, dtype=U64)[b] * U64(m)
    dyadic_bl = np.ldexp(1.0, -(np.arange(n) % 7))
    dyadic = (U64(1) << rng.integers(0, 20, size=(6, n)).astype(U64)) * (rng.random((6, n)) < 0.5).astype(U64)
    dyadic[:, 0] = 1
    return {
        "two identical": (np.stack([x, x, y]), first, bl),
        "three identical": (np.stack([y, x, x, x]), first, bl),
        "two pairs at one distance": (np.stack([leaf(0, 5), leaf(1, 3), leaf(3, 7), leaf(4, 9)]), sym_first, sym_bl),
        "empty first": (np.stack([zero, x, y, z]), first, bl),
        "empty in the middle": (np.stack([x, y, zero, z]), first, bl),
        "empty last": (np.stack([x, y, z, zero]), first, bl),
        "all empty": (np.stack([zero, zero, zero]), first, bl),
        "one not empty": (np.stack([zero, x, zero]), first, bl),
        "dyadic": (dyadic, first, dyadic_bl),
    }


@pytest.mark.parametrize("name", sorted(forged_cohorts()))
def test_forged_cohorts(name):
    mass, first, bl = forged_cohorts()[name]
    want, count = numpy_squash(mass, first, bl)
    records, got_count = host_all_records(mass, first, bl)
    assert got_count == count and records.tobytes() == want.tobytes(), (name, records, want)
    r = records
    if name == "two identical":
        assert (r[0]["a"], r[0]["b"]) == (0, 1) and same_bits([r[0]["dist"], r[0]["len_a"], r[0]["len_b"]], [0.0, 0.0, 0.0])
        assert (r[1]["a"], r[1]["b"]) == (3, 2) and r[1]["dist"] == cohort_mod.kr_host(mass, first, bl)[0, 2]
    elif name == "three identical":       # three zeros: (1, 2) is the earliest pair, then the merged one with 3
        assert [(int(m["a"]), int(m["b"])) for m in r] == [(1, 2), (4, 3), (0, 5)]
        # (the second cluster is 3 x / 3, each plane rounded twice: within a few ulps of x, not x)
        assert same_bits(r["dist"][:2], [0.0, 0.0]) and abs(r[2]["dist"] - cohort_mod.kr_host(mass, first, bl)[0, 1]) <= 1e-12 * r[2]["dist"]
    elif name == "two pairs at one distance":
        kr = cohort_mod.kr_host(mass, first, bl)
        assert kr[0, 1] == kr[2, 3] == 0.375 == kr[~np.eye(4, dtype=bool)].min()
        assert [(int(m["a"]), int(m["b"])) for m in r] == [(0, 1), (2, 3), (4, 5)]
        assert same_bits(r["dist"][:2], [0.375, 0.375]) and same_bits(r["len_a"][:2], [0.1875] * 2) and same_bits(r["len_b"][:2], [0.1875] * 2)
        # each cherry's cluster has half its mass on either leaf: 0.25 * 0.5 + 0.125 * 0.5 for the leaves' halves and
        # 0.0625 * 2 for the inner branch, all of it below both halves, on either side: 0.625; equal weights: half each
        assert same_bits(r[2]["dist"], 0.625) and same_bits([r[2]["len_a"], r[2]["len_b"]], [0.3125, 0.3125])
    elif name.startswith("empty"):
        empty = int(np.flatnonzero(mass.sum(axis=1, dtype=U64) == 0)[0])
        assert count == 2 and empty not in set(r["a"][:2]) | set(r["b"][:2])
    elif name == "all empty":
        assert count == 0 and (r["a"] == NONE).all() and (r["b"] == NONE).all() and not r["dist"].view(U64).any()
    elif name == "one not empty":
        assert count == 0 and (r["a"] == NONE).all() and not r["len_a"].view(U64).any() and not r["len_b"].view(U64).any()


def test_three_samples_on_three_leaves_by_hand():
    # ((0,1)2,(3,4)5)6 with lengths 0.5 0.25 0.125 1 0.5 0.25: A all on leaf 0, B on leaf 1, C on leaf 3.
    first = numpy_first(BALANCED)
    bl = [0.5, 0.25, 0.125, 1.0, 0.5, 0.25, 0.0]
    mass = np.array([[9, 0, 0, 0, 0, 0, 0], [0, 4, 0, 0, 0, 0, 0], [0, 0, 0, 11, 0, 0, 0]], U64)
    records, count = host_all_records(mass, first, bl)
    assert count == 2
    # KR(A, B) = 0.25 + 0.125 = 0.375 (the sisters' midpoints); KR(A, C) = 0.25 + 0.125 + 0.25 + 0.5 = 1.125;
    # KR(B, C) = 0.125 + 0.125 + 0.25 + 0.5 = 1.  The sisters go first; the merged cluster has half its mass on each, and
    # moving half of it along the path takes 0.375 / 2 to either part: all dyadic, exact.
    assert (records[0]["a"], records[0]["b"]) == (0, 1)
    assert same_bits([records[0]["dist"], records[0]["len_a"], records[0]["len_b"]], [0.375, 0.1875, 0.1875])
    # record 1: node 3 = {A, B} (weight 2) with C (weight 1).  KR(m, C) = KR(A, C) / 2 + KR(B, C) / 2 = 1.0625: the
    # two halves travel the same way over the edges they share.  Still dyadic: exact.  The new cluster is
    # (2 m + C) / 3: its parts lie at a third and at two thirds of that distance, len_a = 1.0625 / 3 and
    # len_b = 2 * 1.0625 / 3.  Thirds are rounded: seven terms of at most an ulp each, and the planes' own rounding.
    assert (records[1]["a"], records[1]["b"]) == (3, 2) and same_bits(records[1]["dist"], 1.0625)
    slack = 16 * np.finfo(np.float64).eps * 1.0625
    assert abs(records[1]["len_a"] - 1.0625 / 3) <= slack and abs(records[1]["len_b"] - 2 * 1.0625 / 3) <= slack
    assert_records(cohort_mod.squash_host(mass, first, bl), numpy_squash(mass, first, bl))


def leaves_under(records, num_samples):
    under = [[s] for s in range(num_samples)]
    for m in records:
        under.append(under[int(m["a"])] + under[int(m["b"])])
    return under


def test_properties_on_random_cohorts():
    tree = synth.make_tree(40, seed=7)
    first = numpy_first(tree.parent)
    bl = tree.branch_length
    rng = np.random.default_rng(6)
    for num_samples, empty in ((12, None), (33, 5), (20, 0)):
        mass = random_cells(rng, num_samples, len(first), empty=empty, bits=50)
        live = mass.sum(axis=1, dtype=U64) > 0
        records = cohort_mod.squash_host(mass, first, bl)
        assert len(records) == live.sum() - 1
        under = leaves_under(records, num_samples)
        assert sorted(under[-1]) == list(np.flatnonzero(live))              # every clustered sample once under the root
        kr = cohort_mod.kr_host(mass, first, bl)
        assert records[0]["dist"] == kr[np.ix_(live, live)][~np.eye(live.sum(), dtype=bool)].min()
        # the merged point lies on the segment between its parts: the sum is exact but for rounding
        dist, la, lb = records["dist"], records["len_a"], records["len_b"]
        assert (np.abs(la + lb - dist) <= 1e-9 * dist).all(), np.abs(la + lb - dist).max()
        # ... and divides it inversely to the weights: len_a * w_a = len_b * w_b = dist * w_a * w_b / W.  The weights
        # here are at most 32, so either product is at least dist / 33 of its weight: the same 1e-9 holds relative to it.
        wa = np.array([len(under[int(m["a"])]) for m in records], dtype=np.float64)
        wb = np.array([len(under[int(m["b"])]) for m in records], dtype=np.float64)
        assert (np.abs(la * wa - lb * wb) <= 1e-9 * np.maximum(la * wa, lb * wb)).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_squash_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    names = ("epik_amd_cohort_squash_device", "epik_amd_cohort_squash", "epik_amd_cohort_squash_host")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3 and capi.SQUASH_MERGE.itemsize == 32
    assert [capi.SQUASH_MERGE.fields[k][1] for k in ("a", "b", "dist", "len_a", "len_b")] == [0, 4, 8, 16, 24]
    err = lambda: lib.epik_amd_last_error().decode()
    count = ctypes.c_uint32(0)
    assert lib.epik_amd_cohort_squash_device(None, None, None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_squash(None, None, None, None, ctypes.byref(count)) == capi.ERR_INVALID and "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.ones((2, 3), U64)
    records = np.zeros(1, dtype=capi.SQUASH_MERGE)
    bl = np.array([0.1, 0.2, 0.0])
    args = lambda m=mass, s=2, n=3, f=first, l=bl, r=records: (m.ctypes.data, s, n, f.ctypes.data, l.ctypes.data,
                                                                r.ctypes.data if r is not None else None, ctypes.byref(count))
    host = lib.epik_amd_cohort_squash_host
    assert host(*args()) == capi.OK and count.value == 1 and (records[0]["a"], records[0]["b"]) == (0, 1)
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID
    assert host(None, 2, 3, first.ctypes.data, bl.ctypes.data, records.ctypes.data, ctypes.byref(count)) == capi.ERR_INVALID
    assert host(*args(r=None)) == capi.ERR_INVALID and "null argument" in err()
    assert host(mass.ctypes.data, 2, 3, first.ctypes.data, bl.ctypes.data, records.ctypes.data, None) == capi.ERR_INVALID
    for bad in (-0.1, np.nan, np.inf):
        assert host(*args(l=np.array([0.1, bad, 0.0]))) == capi.ERR_INVALID and "branch 1" in err() and "length" in err()
    above = np.array([0, 2, 0], dtype=np.uint32)
    assert host(*args(f=above)) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
    # one sample: valid, no merge, no record to write
    count.value = 9
    assert host(*args(s=1, r=None)) == capi.OK and count.value == 0
    assert len(cohort_mod.squash_host(mass[:1], first, bl)) == 0
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.squash_host(mass, first, [0.1, -1.0, 0.0])
    with pytest.raises(ValueError):
        cohort_mod.squash_host(mass, first[:2], bl)


# ---- the drivers and the launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_squash_without_cohort_and_name_the_flag(host_bins, tmp_path, binary):
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"),
                          "-o", str(tmp_path), "--cohort-squash"], capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and "--cohort-squash" in run.stderr and "--cohort " in run.stderr, run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(tmp_path.iterdir())
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-squash " in out.stdout and "cohort_squash_<list>.nwk" in out.stdout


def test_launcher_passes_the_flag_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-squash" not in default and epik.driver_command(**kw, cohort_squash=False) == default
    assert "--cohort-squash" not in epik.driver_command(**kw, cohort=True)
    assert epik.driver_command(**kw, cohort=True, cohort_squash=True)[:-1] == default[:-1] + ["--cohort", "--cohort-squash"]
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort_squash=True)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-squash" in out.stdout
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort-squash", me], capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort" in run.stderr, (run.stdout, run.stderr)


def test_the_two_files_read_back_and_quote_names():
    names = ["a", "b c", "d'e", "z.9_-", "none"]
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.array([[5, 0, 0], [0, 7, 0], [0, 0, 3], [1, 1, 1], [0, 0, 0]], U64)
    bl = [0.5, 0.25, 0.1]
    live = mass.sum(axis=1) > 0
    records = cohort_mod.squash_host(mass, first, bl)
    text = cohort_mod.format_squash_tsv(names, live, records)
    lines = text.split("\n")
    assert lines[0] == "# epik_amd squash v1  samples=5 clustered=4 merges=3" and lines[1] == "# unclustered\tnone"
    assert lines[2] == "step\tnode\ta\tb\tsize\tdist\tlen_a\tlen_b" and len(lines) == 7 and lines[-1] == ""
    assert lines[3].split("\t")[:2] == ["0", "5"] and lines[5].split("\t")[4] == "4"
    assert lines[3].split("\t")[5] == "%.17g" % records[0]["dist"]
    import tempfile
    with tempfile.TemporaryDirectory() as folder:
        path = os.path.join(folder, "cohort_squash_x.tsv")
        with open(path, "w", newline="") as fh:
            fh.write(text)
        back, info = cohort_mod.read_squash_tsv(path)
        with open(path, "w") as fh:
            fh.write("# something else\n")
        with pytest.raises(ValueError):
            cohort_mod.read_squash_tsv(path)
    assert back.tobytes() == records.tobytes()                                # %.17g reads back to the same double
    assert info["samples"] == 5 and info["clustered"] == 4 and info["merges"] == 3 and info["unclustered"] == ["none"]
    assert list(info["node"]) == [5, 6, 7] and info["size"][-1] == 4
    assert cohort_mod.format_squash_tsv(names, live, back) == text
    # the tree: child a before child b, %.17g, no length at the root, quoted where a character is outside [A-Za-z0-9_.-]
    nwk = cohort_mod.format_squash_newick(names, live, records)
    assert nwk.endswith(");\n") and nwk.count("(") == 3 and "none" not in nwk
    assert "'b c':" in nwk and "'d''e':" in nwk and "z.9_-:" in nwk and "'z.9_-'" not in nwk and "a:" in nwk
    label = {0: "a", 1: "'b c'", 2: "'d''e'", 3: "z.9_-"}
    text_of = dict(label)
    for t, m in enumerate(records):
        text_of[5 + t] = "(%s:%.17g,%s:%.17g)" % (text_of[int(m["a"])], m["len_a"], text_of[int(m["b"])], m["len_b"])
    assert nwk == text_of[7] + ";\n"
    none = records[:0]
    assert cohort_mod.format_squash_newick(["x y", "q"], [True, False], none) == "'x y';\n"
    assert cohort_mod.format_squash_newick(["x y", "q"], [False, False], none) == ";\n"
    assert cohort_mod.format_squash_tsv(["x y", "q"], [False, False], none) == (
        "# epik_amd squash v1  samples=2 clustered=0 merges=0\n# unclustered\tx y\n# unclustered\tq\n"
        "step\tnode\ta\tb\tsize\tdist\tlen_a\tlen_b\n")


# ---- the host code stand-alone -----------------------------------------------------------------------------------------
def _squash_input(path, mass, first, bl):
    with open(path, "wb") as fh:
        fh.write(np.array(mass.shape, dtype="<u8").tobytes() + np.ascontiguousarray(mass, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(bl, np.float64).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_squash_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, bl = tree_case("tree15")
    first = numpy_first(parent)
    cases = {"random": random_cells(np.random.default_rng(9), 7, len(parent), empty=3), "one": random_cells(np.random.default_rng(9), 1, len(parent)),
             "empty": np.zeros((3, len(parent)), U64)}
    for name, mass in cases.items():
        _squash_input(tmp_path / "in.bin", mass, first, bl)
        run = subprocess.run([binary, "squash", str(tmp_path / "out.bin"), str(tmp_path / "in.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (name, run.stderr)
        raw = (tmp_path / "out.bin").read_bytes()
        want, count = host_all_records(mass, first, bl)
        assert raw == want.tobytes() + np.uint32(count).tobytes(), name
    bad = bl.copy()
    bad[4] = -0.5
    _squash_input(tmp_path / "bad.bin", cases["random"], first, bad)
    run = subprocess.run([binary, "squash", str(tmp_path / "o.bin"), str(tmp_path / "bad.bin")], capture_output=True, text=True)
    assert run.returncode == 1 and "branch 4" in run.stderr
