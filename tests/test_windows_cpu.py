"""Painting by windows without a device: the window geometry (Python against the header's inline function, compiled
as C), the groups at a rank, epik_amd_windows_paint_host against the numpy restatement bit for bit, the breakpoints and
the files."""
import os
import subprocess

import numpy as np
import pytest

from epik_amd import capi, synth, taxonomy, windows
from test_assign_cpu import forged_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, W = 8, 40
STEPS = (1, 7, W)


def geometry_lengths(k, w, s):
    return sorted({0, 1, k - 1, k, w - 1, w, w + 1, w + s - 1, w + s, w + s + 1})


def hand_spans(length, w, s):
    """The windows of the issue's wording, one after the other."""
    if length <= w:
        return [(0, length)]
    nw = 1 + -(-(length - w) // s)
    return [(i * s, i * s + w) for i in range(nw - 1)] + [(length - w, length)]


@pytest.mark.parametrize("step", STEPS)
def test_geometry_in_python(step):
    for length in geometry_lengths(K, W, step) + [5000]:
        want = hand_spans(length, W, step)
        assert windows.window_count(length, W, step) == len(want)
        assert [windows.window_span(length, W, step, w) for w in range(len(want))] == want
        # the tail is covered, no window is longer than W, no gap between neighbours
        assert want[-1][1] == length and all(e - b == min(length, W) for b, e in want)
        assert all(b1 <= e0 and b1 > b0 for (b0, e0), (b1, _) in zip(want, want[1:]))
        with pytest.raises(IndexError):
            windows.window_span(length, W, step, len(want))
    lens = geometry_lengths(K, W, step)
    offs = windows.win_offsets(lens, W, step)
    assert offs.dtype == np.uint64 and offs[0] == 0
    assert np.array_equal(np.diff(offs.astype(np.int64)), [len(hand_spans(x, W, step)) for x in lens])
    for bad in ((0, 1), (W, 0), (W, W + 1), (1 << 31, 1)):
        with pytest.raises(ValueError):
            windows.window_count(10, *bad)


C_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "epik_amd.h"
int main(int argc, char **argv)
{
    const uint32_t window = (uint32_t)strtoul(argv[1], 0, 10), step = (uint32_t)strtoul(argv[2], 0, 10);
    for (int a = 3; a < argc; ++a) {
        const uint64_t len = strtoull(argv[a], 0, 10), nw = epik_amd_window_span(len, window, step, 0, 0, 0);
        printf("%llu", (unsigned long long)nw);
        for (uint64_t w = 0; w < nw; ++w) {
            uint64_t b = 77, e = 77;
            epik_amd_window_span(len, window, step, w, &b, &e);
            printf(" %llu %llu", (unsigned long long)b, (unsigned long long)e);
        }
        uint64_t b = 77, e = 78;  /* beyond the last window nothing is written */
        epik_amd_window_span(len, window, step, nw, &b, &e);
        printf(" %llu %llu\n", (unsigned long long)b, (unsigned long long)e);
    }
    return 0;
}
"""


def test_geometry_of_the_header_equals_python(tmp_path):
    src, exe = tmp_path / "span.c", tmp_path / "span"
    src.write_text(C_PROGRAM)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    for step in STEPS:
        lens = geometry_lengths(K, W, step) + [5000]
        out = subprocess.run([str(exe), str(W), str(step)] + [str(x) for x in lens], check=True, capture_output=True, text=True)
        for length, line in zip(lens, out.stdout.strip().split("\n")):
            f = [int(x) for x in line.split()]
            want = hand_spans(length, W, step)
            assert f[0] == len(want) and f[-2:] == [77, 78]
            assert list(zip(f[1:-2:2], f[2:-2:2])) == want, (length, step)
    out = subprocess.run([str(exe), "0", "1", "10"], check=True, capture_output=True, text=True)
    assert out.stdout.split()[0] == "0"
    out = subprocess.run([str(exe), "10", "11", "10"], check=True, capture_output=True, text=True)
    assert out.stdout.split()[0] == "0"


def test_geometry_of_the_library_equals_python():
    import ctypes
    lib = capi.load()
    for step in STEPS:
        for length in geometry_lengths(K, W, step) + [5000, 1 << 40]:
            nw = lib.epik_amd_window_span(length, W, step, 0, None, None)
            assert nw == windows.window_count(length, W, step)
            for w in sorted(w for w in {0, 1, nw // 2, nw - 2, nw - 1} if 0 <= w < nw):
                b, e = ctypes.c_uint64(77), ctypes.c_uint64(77)
                assert lib.epik_amd_window_span(length, W, step, w, ctypes.byref(b), ctypes.byref(e)) == nw
                assert (b.value, e.value) == windows.window_span(length, W, step, w)
    assert lib.epik_amd_window_span(10, 0, 1, 0, None, None) == 0 and lib.epik_amd_window_span(10, 1 << 31, 1, 0, None, None) == 0
    assert lib.epik_amd_window_span(10, 5, 6, 0, None, None) == 0 and lib.epik_amd_window_span(10, 5, 0, 0, None, None) == 0


def test_slice_windows():
    data, offs = synth.pack_reads(["ACGTACGTAC", "", "ACG", "ACGTACGTACGTA"])
    wdata, woffs, wo = windows.slice_windows(data, offs, 4, 3)
    got = [bytes(wdata[int(woffs[i]):int(woffs[i + 1])]).decode() for i in range(len(woffs) - 1)]
    assert got == ["ACGT", "TACG", "GTAC", "", "ACG", "ACGT", "TACG", "GTAC", "CGTA"]
    assert list(wo) == [0, 3, 4, 5, 9]


# ---- groups ------------------------------------------------------------------------------------------------------

def _depths(taxa):
    d = np.zeros(taxa.num_taxa, np.int64)
    for t in range(taxa.num_taxa - 2, -1, -1):
        d[t] = d[taxa.parent[t]] + 1
    return d


@pytest.mark.parametrize("leaves,ranks", [(8, 2), (60, 3), (200, 4)])
def test_groups_at_rank(leaves, ranks):
    tree = synth.make_tree(leaves, seed=leaves)
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, ranks))
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    depth = _depths(taxa)
    for d in (1, 2):
        group, group_taxa = taxonomy.groups_at_rank(taxa, label, d)
        assert group.dtype == np.uint32 and group_taxa == sorted(group_taxa)
        assert [depth[t] for t in group_taxa] == [d] * len(group_taxa)
        assert group_taxa == [t for t in range(taxa.num_taxa) if depth[t] == d]
        for b in range(tree.num_nodes):       # by steps up the taxonomy
            t = int(label[b])
            if depth[t] < d:
                assert group[b] == capi.WINDOW_NO_GROUP
                continue
            while depth[t] > d:
                t = int(taxa.parent[t])
            assert group_taxa[int(group[b])] == t
        assert group[tree.num_nodes - 1] == capi.WINDOW_NO_GROUP or len(group_taxa) == 1    # the root branch lies above
    group, group_taxa = taxonomy.groups_at_rank(taxa, label, int(depth.max()) + 1)
    assert group_taxa == [] and (group == capi.WINDOW_NO_GROUP).all()
    with pytest.raises(ValueError):
        taxonomy.groups_at_rank(taxa, label, 0)


# ---- the rule ----------------------------------------------------------------------------------------------------

def groupings(num_branches):
    b = np.arange(num_branches)
    return {"all-one": np.zeros(num_branches, np.uint32), "all-none": np.full(num_branches, capi.WINDOW_NO_GROUP, np.uint32),
            "alternating": (b % 2).astype(np.uint32), "quarters": (b * 4 // num_branches).astype(np.uint32),
            "some-none": np.where(b % 3 == 0, capi.WINDOW_NO_GROUP, b % 5).astype(np.uint32)}


def random_win_offsets(rng, total, n):
    cuts = np.sort(rng.integers(0, total + 1, size=n - 1))
    return np.concatenate([[0], cuts, [total]]).astype(np.uint64)


def same_paint(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


TAUS = ((1 << 29) + 1, int(np.rint(0.8 * 2 ** 30)), 1 << 30)


@pytest.mark.parametrize("keep", [1, 2, 7, 63, 64])
def test_paint_host_equals_numpy_on_forged_rows(keep):
    rng = np.random.default_rng(keep)
    N, V = 59, 700
    rows, n_rows, counts = forged_batch(rng, V, keep, N)
    wo = random_win_offsets(rng, V, 23)
    seen = set()
    for name, group in groupings(N).items():
        for tau_q in TAUS:
            want = windows.numpy_paint(rows, n_rows, counts, wo, group, tau_q)
            got = windows.paint_host(rows, n_rows, counts, wo, group, tau_q)
            assert same_paint(got, want), (name, tau_q)
            seen |= set(int(c) for c in want[0]["call"])
            assert int(want[2].sum()) == sum(1 for i in range(23) for v in range(int(wo[i]), int(wo[i + 1]))
                                             if v == int(wo[i]) or want[0]["call"][v] != want[0]["call"][v - 1])
    assert set(capi.WINDOW_CLASSES) <= seen and min(seen) < capi.WINDOW_AMBIGUOUS


def test_hand_windows():
    keep, N = 3, 6
    rows = np.zeros((5, keep), dtype=capi.PLACEMENT)
    rows["branch"] = [[0, 1, 4], [4, 5, 0], [0, 4, 2], [5, 5, 5], [2, 0, 0]]
    rows["lwr"] = [[0.5, 0.25, 0.25], [0.5, 0.25, 0.25], [0.5, 0.5, 0.0], [0.25, 0.25, 0.5], [0.75, 0.25, 0]]
    n_rows, counts = np.full(5, 3, np.uint32), np.ones((5, keep), np.uint32)
    group = np.array([0, 0, capi.WINDOW_NO_GROUP, 7, 1, 1], np.uint32)
    wo = np.array([0, 5], np.uint64)
    rec, seg, ns = windows.numpy_paint(rows, n_rows, counts, wo, group, 3 << 28)
    q = 1 << 30
    assert [tuple(int(x) for x in r) for r in rec] == [
        (0, 3 * q // 4, 0, q), (1, 3 * q // 4, 1, q), (capi.WINDOW_AMBIGUOUS, 0, 0, 0), (1, q, 1, q), (capi.WINDOW_AMBIGUOUS, 0, 0, 0)]
    assert int(ns[0]) == 5 and [int(s["first_window"]) for s in seg] == [0, 1, 2, 3, 4]
    # tau 3/4 + 1 quantum: the first two windows miss it; NO_GROUP holds the majority of the last and is never called
    rec2, seg2, ns2 = windows.numpy_paint(rows, n_rows, counts, wo, group, (3 << 28) + 1)
    assert [int(c) for c in rec2["call"]] == [capi.WINDOW_AMBIGUOUS] * 3 + [1, capi.WINDOW_AMBIGUOUS]
    assert int(ns2[0]) == 3 and [(int(s["first_window"]), int(s["num_windows"])) for s in seg2[:3]] == [(0, 3), (3, 1), (4, 1)]
    assert seg2[3:].tobytes() == bytes(64)
    assert (int(seg2[1]["call_mass"]), int(seg2[1]["total"])) == (q, q) and int(seg2[0]["total"]) == 0
    for tau in (3 << 28, (3 << 28) + 1):
        assert same_paint(windows.paint_host(rows, n_rows, counts, wo, group, tau), windows.numpy_paint(rows, n_rows, counts, wo, group, tau))


def test_sums_do_not_saturate_in_the_segments():
    keep, V = 64, 9
    rows = np.zeros((V, keep), dtype=capi.PLACEMENT)
    rows["lwr"] = 1.0
    n_rows, counts = np.full(V, keep, np.uint32), np.ones((V, keep), np.uint32)
    group = np.zeros(1, np.uint32)
    got = windows.paint_host(rows, n_rows, counts, np.array([0, V], np.uint64), group, 1 << 30)
    assert (got[0]["call_mass_q"] == 0xFFFFFFFF).all() and (got[0]["total_q"] == 0xFFFFFFFF).all()
    assert int(got[2][0]) == 1 and int(got[1][0]["call_mass"]) == int(got[1][0]["total"]) == V * keep << 30
    assert same_paint(got, windows.numpy_paint(rows, n_rows, counts, np.array([0, V], np.uint64), group, 1 << 30))


def test_paint_host_refusals():
    rows, n_rows, counts = forged_batch(np.random.default_rng(0), 16, 3, 10)
    wo, group = np.array([0, 16], np.uint64), np.zeros(10, np.uint32)
    for tau_q in (0, 1 << 29, (1 << 30) + 1):
        with pytest.raises(capi.EpikAmdError, match=r"tau_q must lie in \(2\^29, 2\^30\]"):
            windows.paint_host(rows, n_rows, counts, wo, group, tau_q)
    with pytest.raises(capi.EpikAmdError, match="win_offsets not monotone"):
        windows.paint_host(rows, n_rows, counts, np.array([0, 9, 5, 16], np.uint64), group, 1 << 30)
    group[4] = capi.WINDOW_AMBIGUOUS
    with pytest.raises(capi.EpikAmdError, match="branch 4: its group id is a status code"):
        windows.paint_host(rows, n_rows, counts, wo, group, 1 << 30)
    with pytest.raises(ValueError):
        windows.tau_q_of(0.5)
    assert windows.tau_q_of(0.8) == TAUS[1] and windows.tau_q_of(1) == 1 << 30


# ---- breakpoints and files ---------------------------------------------------------------------------------------

def hand_segments(spec):
    seg = np.zeros(len(spec), dtype=capi.WINDOW_SEGMENT)
    first = 0
    for s, (call, num, mass, total) in enumerate(spec):
        seg[s] = (call, first, num, 0, mass, total)
        first += num
    return seg


def test_breakpoints_on_hand_segments():
    A, NH = capi.WINDOW_AMBIGUOUS, capi.WINDOW_NO_HIT
    L, w, s = 1000, 100, 25          # 37 windows, the last one [900, 1000)
    assert windows.window_count(L, w, s) == 37
    seg = hand_segments([(2, 10, 9, 10), (A, 2, 0, 0), (0, 5, 4, 5), (NH, 3, 0, 0), (0, 4, 4, 4), (A, 1, 0, 0), (1, 12, 12, 12)])
    # 2 -> 0 over the ambiguous windows 10, 11: from the start of window 9 to the end of window 12
    # 0 -> 0 over the no-hit run: no breakpoint;  0 -> 1: from window 23 to window 25
    assert windows.breakpoints(seg, L, w, s) == [(2, 0, 225, 400), (0, 1, 575, 725)]
    assert windows.breakpoints(seg[:2], L, w, s) == [] and windows.breakpoints(seg[3:4], L, w, s) == []
    assert windows.segment_span(seg[6], L, w, s) == (625, 1000) and windows.segment_span(seg[0], L, w, s) == (0, 325)
    # neighbours without a gap
    seg = hand_segments([(0, 19, 1, 1), (3, 18, 1, 1)])
    assert windows.breakpoints(seg, L, w, s) == [(0, 3, 450, 575)]


def test_files_round_trip():
    A = capi.WINDOW_AMBIGUOUS
    paths = ["Bacteria;Firmicutes", "Bacteria;Proteobacteria", "Archaea;Euryarchaeota"]
    names, lengths, w, s = ["chimera one", "short", "plain"], [1000, 60, 300], 100, 25
    wo = windows.win_offsets(lengths, w, s)
    assert list(wo) == [0, 37, 38, 47]
    segments = np.zeros(47, dtype=capi.WINDOW_SEGMENT)
    segments[0:3] = hand_segments([(0, 18, 17 << 30, 18 << 30), (A, 1, 0, 0), (2, 18, 12345678901, 18 << 30)])
    segments[37] = (capi.WINDOW_TOO_SHORT, 0, 1, 0, 0, 0)
    segments[38] = (1, 0, 9, 0, 1, 3)
    n_segments = np.array([3, 1, 1], np.uint32)
    tau_q = windows.tau_q_of(0.8)
    text = windows.format_windows_tsv(names, lengths, wo, segments, n_segments, paths, w, s, tau_q, rank=2)
    lines = text.split("\n")
    assert lines[0] == f"# epik_amd windows v1\twindow=100\tstep=25\ttau_q={tau_q}\tgroups=3\trank=2\trecords=3"
    assert lines[1:4] == [f"# group\t{g}\t{p}" for g, p in enumerate(paths)]
    assert lines[4] == "name\tsegment\tstart\tend\twindows\tcall\tsupport"
    assert lines[5] == "chimera one\t0\t0\t525\t18\tBacteria;Firmicutes\t" + "%.17g" % (17 / 18)
    assert lines[6] == "chimera one\t1\t450\t550\t1\tambiguous\tNA"
    assert lines[8] == "short\t0\t0\t60\t1\ttoo_short\tNA"
    assert lines[9] == "plain\t0\t0\t300\t9\tBacteria;Proteobacteria\t" + "%.17g" % (1 / 3) and lines[10:] == [""]
    back = windows.read_windows_tsv(text)
    assert back["header"] == {"window": 100, "step": 25, "tau_q": tau_q, "groups": 3, "rank": 2, "records": 3}
    assert back["groups"] == paths and len(back["segments"]) == 5
    assert back["segments"][2] == ("chimera one", 2, 475, 1000, 18, paths[2], 12345678901 / (18 << 30))
    assert back["segments"][3] == ("short", 0, 0, 60, 1, "too_short", None)
    bp = windows.format_breakpoints_tsv(names, lengths, wo, segments, n_segments, paths, w, s)
    assert bp == f"name\tleft\tright\tfrom\tto\nchimera one\t{paths[0]}\t{paths[2]}\t425\t575\n"
    with pytest.raises(ValueError, match="not a windows file"):
        windows.read_windows_tsv("name\tsegment\n")
    with pytest.raises(ValueError, match="line 7: 7 columns expected"):
        windows.read_windows_tsv("\n".join(lines[:6] + ["x\ty"]) + "\n")
