"""Painting by windows on the GPU (epik_amd_placer_place_windows[_device], epik_amd_windows_paint_device;
Placer.place_windows, Placer.paint_windows): the windows' rows bit-exact against the CPU oracle run on host-sliced
windows, the same bytes whatever the chunks, the records and segments bit for bit against numpy and the host mirror,
and chimeras of two references found where they were joined."""
import numpy as np
import pytest

from conftest import assert_rows_match, select_kernel
from epik_amd import capi, synth, windows
from test_assign_cpu import forged_batch
from test_strand_gpu import both_rule, rc_packed
from test_windows_cpu import TAUS, geometry_lengths, groupings, same_paint

pytestmark = pytest.mark.gpu

KERNELS = ["default", "packed", "team4"]
K = 6
WINDOWS = [K, 15, 16, 17, 63, 64, 65, 100]
TAU = TAUS[1]          # 0.8


def steps_of(w):
    return sorted({1, min(7, w), w})


@pytest.fixture(params=KERNELS)
def kernel(request, monkeypatch):
    if request.param != "default":
        select_kernel(monkeypatch, request.param)
    return request.param


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


@pytest.fixture(scope="module")
def case59():
    tree = synth.make_tree(30, seed=3)
    return synth.make_db(tree.num_nodes, kmer_size=K, p_present=0.7, seed=7, lognormal=(1.5, 1.0))


def batch_for(w, s, seed):
    """Reads of every length at which the geometry changes, of odd lengths packed together (windows start at every
    residue mod 16), dirty ones (IUPAC, gaps, lower case) and one of 5 000 characters."""
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), size=n)) for n in geometry_lengths(K, w, s)]
    reads += ["".join(rng.choice(list("ACGT"), size=w + 2 * s + 1 + 2 * i)) for i in range(17)]
    dirty = ["".join(rng.choice(list("ACGTNRYKMSWBDHV-"), size=w + 3 * s + i)) for i in range(6)]
    reads += [r.lower() if i % 2 else r for i, r in enumerate(dirty)]
    reads += ["".join(rng.choice(list("ACGT"), size=5000)), "acgtRYKMBVDHSWN" * 9, "-" * (w + 1), "ACGT" * 30]
    return synth.pack_reads(reads)


_REFERENCE = {}


def oracle_windows(oracle_lib, db, data, offs, w, s, mode, key=None):
    """What place_windows must give: the oracle on the host-sliced windows, for `both` the strand rule on two runs."""
    if key is not None and (key, mode) in _REFERENCE:
        return _REFERENCE[(key, mode)]
    orc = oracle_lib.Oracle.from_synth(db)
    wdata, woffs, wo = windows.slice_windows(data, offs, w, s)
    fwd = orc.place(wdata, woffs, num_threads=0) if mode != "reverse" else None
    rev = orc.place(*rc_packed(wdata, woffs), num_threads=0) if mode != "forward" else None
    if mode == "forward":
        out = (fwd, np.zeros(len(woffs) - 1, np.uint8), wo)
    elif mode == "reverse":
        out = (rev, np.ones(len(woffs) - 1, np.uint8), wo)
    else:
        out = (*both_rule(fwd, rev), wo)
    if key is not None:
        _REFERENCE[(key, mode)] = out
    return out


@pytest.mark.parametrize("w", WINDOWS)
def test_windows_equal_the_oracle_on_host_sliced_windows(placer_cls, oracle_lib, case59, kernel, w):
    with placer_cls.from_synth(case59) as pl:
        for s in steps_of(w):
            data, offs = batch_for(w, s, seed=100 * w + s)
            for mode in ("both", "forward", "reverse") if s == min(7, w) else ("both",):
                want, want_strand, want_wo = oracle_windows(oracle_lib, case59, data, offs, w, s, mode, key=(w, s))
                rows, n, counts, strand, wo = pl.place_windows(data, offs, w, s, mode)
                assert np.array_equal(wo, want_wo), (w, s, mode)
                assert (n != capi.ROWS_COUNTS_TOO_NARROW).all()
                assert_rows_match(rows, n, counts, *want)
                assert np.array_equal(strand, want_strand), (w, s, mode)
                if mode == "both" and w >= 15:
                    assert 0 < int(strand.sum()) < len(strand)


def test_chunks_give_identical_bytes(placer_cls, case59, monkeypatch):
    data, offs = batch_for(17, 7, seed=5)
    with placer_cls.from_synth(case59) as pl:
        monkeypatch.delenv("EPIK_AMD_WINDOW_CHUNK_WINDOWS", raising=False)
        want = pl.place_windows(data, offs, 17, 7, "both")
        assert int(want[4][-1]) > 65 * 3
        for chunk in (1, 64, 65):
            monkeypatch.setenv("EPIK_AMD_WINDOW_CHUNK_WINDOWS", str(chunk))
            got = pl.place_windows(data, offs, 17, 7, "both")
            assert same_paint(got, want), chunk


def test_device_entry_on_a_side_stream(placer_cls, case59):
    import torch
    w, s = 64, 7
    data, offs = batch_for(w, s, seed=6)
    lens = np.diff(offs.astype(np.int64))
    wo = windows.win_offsets(lens, w, s)
    total = int(wo[-1])
    wbytes = int((np.diff(wo.astype(np.int64)) * np.minimum(lens, w)).sum())
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(case59) as pl:
        want = pl.place_windows(data, offs, w, s, "both")
        dev, keep, n = torch.device("cuda", pl.device), pl.keep_at_most, len(offs) - 1
        pl.choose_counts(w)
        for mode, with_offsets in (("both", True), ("forward", False)):
            if mode == "forward":
                want = pl.place_windows(data, offs, w, s, "forward")
                pl.choose_counts(w)
            d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
            d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
            d_rows = torch.zeros(total * keep * 2, dtype=torch.float64, device=dev)
            d_n = torch.zeros(total, dtype=torch.int32, device=dev)
            d_counts = torch.zeros(total * keep, dtype=torch.int32, device=dev)
            d_strand = torch.full((total,), 7, dtype=torch.uint8, device=dev)
            d_wo = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
            ws = pl.window_workspace_bytes(n, total, wbytes, mode)
            assert ws >= wbytes + 8 * (total + 1)
            d_ws = torch.zeros(ws, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            pl.place_windows_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, w, s, mode, total, wbytes, d_ws.data_ptr(), ws,
                                    d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_strand.data_ptr(),
                                    d_wo.data_ptr() if with_offsets else 0, stream.cuda_stream)
            stream.synchronize()
            got = (d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(total, keep), d_n.cpu().numpy().view(np.uint32),
                   d_counts.cpu().numpy().view(np.uint32).reshape(total, keep), d_strand.cpu().numpy())
            assert same_paint(got, want[:4]), mode
            if with_offsets:
                assert np.array_equal(d_wo.cpu().numpy().view(np.uint64), wo)
            else:
                assert (d_wo.cpu().numpy() == -1).all()
        with pytest.raises(capi.EpikAmdError, match="workspace smaller than epik_amd_placer_window_workspace_bytes"):
            pl.place_windows_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, w, s, "forward", total, wbytes, d_ws.data_ptr(), ws - 256,
                                    d_rows.data_ptr(), d_n.data_ptr())


def test_refusals(placer_cls, case59):
    data, offs = synth.pack_reads(["ACGTACGTACGT"])
    with placer_cls.from_synth(case59) as pl:
        with pytest.raises(capi.EpikAmdError, match=r"the window must hold a k-mer and be shorter than 2\^31"):
            pl.place_windows(data, offs, K - 1, 1)
        with pytest.raises(capi.EpikAmdError, match=r"the window step must lie in \[1, window\]"):
            pl.place_windows(data, offs, K, K + 1)
        with pytest.raises(capi.EpikAmdError, match="strand mode must be FORWARD, REVERSE or BOTH"):
            pl.place_windows(data, offs, K, 1, 3)
        rows, n, counts, strand, wo = pl.place_windows(*synth.pack_reads([]), K, 1)
        assert len(n) == 0 and list(wo) == [0]
    aa = synth.make_db(59, states="amino", kmer_size=3, p_present=0.5, seed=9)
    pdata, poffs = synth.pack_reads(["MKVLAAGIVGLWRS" * 3, "MK", ""])
    with placer_cls.from_synth(aa) as pl:
        with pytest.raises(capi.EpikAmdError, match="strand placement needs a nucleotide placer"):
            pl.place_windows(pdata, poffs, 10, 5, "both")
        rows, n, counts, strand, wo = pl.place_windows(pdata, poffs, 10, 5, "forward")
        wdata, woffs, want_wo = windows.slice_windows(pdata, poffs, 10, 5)
        want = pl.place_packed(wdata, woffs)
        assert np.array_equal(wo, want_wo) and not strand.any()
        assert same_paint((rows, n, counts), want)


# ---- painting ----------------------------------------------------------------------------------------------------

def assert_paint(pl, rows, n_rows, counts, wo, group, tau_q):
    want = windows.numpy_paint(rows, n_rows, counts, wo, group, tau_q)
    got = pl.paint_windows(rows, n_rows, counts, wo, group, tau_q)
    for what, g, w in zip(("records", "segments", "n_segments"), got, want):
        at = np.flatnonzero(g != w)
        assert len(at) == 0, f"the device's {what} differ from numpy's at {at[:8]}: {g[at[:4]]} for {w[at[:4]]}"
    assert same_paint(got, want), "the device differs from numpy"
    assert same_paint(windows.paint_host(rows, n_rows, counts, wo, group, tau_q), want), "the host mirror differs from numpy"
    return want


NWS = [1, 2, 63, 64, 65, 127, 128, 129, 200]


def test_paint_on_the_rows_the_placement_left(placer_cls, case59):
    rng = np.random.default_rng(8)
    # reads of nw windows each, at W = 16, S = 3: L = W + (nw - 1) S
    reads = ["".join(rng.choice(list("ACGTN"), size=16 + (nw - 1) * 3, p=[.24, .24, .24, .24, .04])) for nw in NWS]
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(case59) as pl:
        rows, n, counts, strand, wo = pl.place_windows(data, offs, 16, 3, "forward")
        assert list(np.diff(wo.astype(np.int64))) == NWS
        for name, group in groupings(59).items():
            want = assert_paint(pl, rows, n, counts, wo, group, TAU)
            if name == "all-one":       # every window with mass is called for the one group
                assert ((want[0]["call"] == 0) == (want[0]["total_q"] > 0)).all() and (want[0]["call"] == 0).sum() > 100
            elif name == "all-none":
                assert (want[0]["call"] >= capi.WINDOW_AMBIGUOUS).all()


@pytest.mark.parametrize("keep", [1, 7, 64])
def test_paint_on_forged_rows(placer_cls, case59, keep):
    rng = np.random.default_rng(keep)
    N = 399
    with placer_cls.from_synth(case59) as pl:
        for n in (1, 63, 64, 65):
            nws = [NWS[(i + n) % len(NWS)] for i in range(n)]
            wo = np.concatenate([[0], np.cumsum(nws)]).astype(np.uint64)
            rows, n_rows, counts = forged_batch(rng, int(wo[-1]), keep, N)
            for name, group in list(groupings(N).items())[2:]:
                for tau_q in TAUS if n == 65 else (TAU,):
                    assert_paint(pl, rows, n_rows, counts, wo, group, tau_q)


def planted_calls(calls, keep=3):
    """One row of all the mass on branch calls[v]: with group[b] = b the call of window v is calls[v]."""
    rows = np.zeros((len(calls), keep), dtype=capi.PLACEMENT)
    rows["branch"][:, 0], rows["lwr"][:, 0] = calls, 1.0
    return rows, np.ones(len(calls), np.uint32), np.ones((len(calls), keep), np.uint32)


def test_runs_that_end_around_a_multiple_of_64(placer_cls, case59):
    N = 300
    group = np.arange(N, dtype=np.uint32)
    reads = []
    for first in (63, 64, 65, 127, 128, 129, 191, 192, 193):       # a run of `first` windows, then one of 70, then one window
        reads.append([0] * first + [1] * 70 + [2])
    for a, b in ((64, 64), (1, 63), (63, 1), (128, 1), (1, 128)):
        reads.append([5] * a + [6] * b)
    reads.append([7] * 200)                                           # all windows equal
    reads.append([7] * 64)
    reads.append(list(range(200)))                                    # every window different
    reads.append([v % 2 for v in range(129)])
    wo = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    rows, n_rows, counts = planted_calls(np.concatenate(reads))
    n_rows[int(wo[9]) + 10] = 0                                       # a status call inside a run splits it
    with placer_cls.from_synth(case59) as pl:
        rec, seg, ns = assert_paint(pl, rows, n_rows, counts, wo, group, 1 << 30)
    assert list(ns[:9]) == [3] * 9 and list(ns[9:]) == [4, 2, 2, 2, 2, 1, 1, 200, 129]
    assert [int(seg[int(wo[i])]["num_windows"]) for i in range(9)] == [63, 64, 65, 127, 128, 129, 191, 192, 193]
    assert all(int(seg[int(wo[i]) + 1]["num_windows"]) == 70 and int(seg[int(wo[i]) + 2]["first_window"]) == f + 70
               for i, f in enumerate((63, 64, 65, 127, 128, 129, 191, 192, 193)))
    assert int(seg[int(wo[14])]["call_mass"]) == 200 << 30 == int(seg[int(wo[14])]["total"])
    # slots beyond n_segments stay zero
    for i in range(len(reads)):
        assert seg[int(wo[i]) + int(ns[i]):int(wo[i + 1])].tobytes() == bytes(32 * (len(reads[i]) - int(ns[i])))


# ---- planted recombinants ----------------------------------------------------------------------------------------

CHIMERA_N, CHIMERA_AT, CHIMERA_W, CHIMERA_S = 399, 600, 120, 30


def chimera_group():
    return (np.arange(CHIMERA_N) * 4 // CHIMERA_N).astype(np.uint32)


@pytest.fixture(scope="module")
def chimera_case():
    return synth.make_clade_db(CHIMERA_N, kmer_size=8, n_refs=40, ref_length=1200, width=(2.0, 0.4), seed=47)


def eligible_pairs(centres, draws=40, seed=1):
    """Seeded draws of two references whose centres lie in different groups, at least 60 branches apart and at least
    15 branches from a group border."""
    group = chimera_group().astype(np.int64)
    rng = np.random.default_rng(seed)
    inside = lambda c: group[max(c - 15, 0)] == group[c] == group[min(c + 15, CHIMERA_N - 1)]
    out = []
    for _ in range(draws):
        a, b = (int(x) for x in rng.choice(len(centres), size=2, replace=False))
        ca, cb = int(centres[a]), int(centres[b])
        if group[ca] != group[cb] and abs(ca - cb) >= 60 and inside(ca) and inside(cb) and (a, b) not in out:
            out.append((a, b))
    return out


def chimeras(refs, pairs):
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [bytes(np.concatenate([chars[refs[a][:CHIMERA_AT]], chars[refs[b][CHIMERA_AT:]]])).decode() for a, b in pairs]


def check_chimeras(pairs, centres, lengths, wo, segments, n_segments):
    """The condition on every chimera: first called segment a's group, last called segment b's, no third group, and the
    join inside the breakpoint's [from, to)."""
    group = chimera_group()
    wo = wo.astype(np.int64)
    for i, (a, b) in enumerate(pairs):
        segs = segments[wo[i]:wo[i] + int(n_segments[i])]
        called = [int(s["call"]) for s in segs if int(s["call"]) < capi.WINDOW_AMBIGUOUS]
        ga, gb = int(group[centres[a]]), int(group[centres[b]])
        assert called and called[0] == ga and called[-1] == gb, (i, a, b, called)
        assert set(called) == {ga, gb}, (i, a, b, called)
        bps = windows.breakpoints(segs, int(lengths[i]), CHIMERA_W, CHIMERA_S)
        assert any(left == ga and right == gb and lo <= CHIMERA_AT < hi for left, right, lo, hi in bps), (i, a, b, bps)


def test_planted_recombinants_are_found_where_they_were_joined(placer_cls, chimera_case):
    db, refs, centres = chimera_case
    pairs = eligible_pairs(centres)
    assert len(pairs) >= 10
    data, offs = synth.pack_reads(chimeras(refs, pairs))
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, strand, wo = pl.place_windows(data, offs, CHIMERA_W, CHIMERA_S, "forward")
        rec, seg, ns = pl.paint_windows(rows, n, counts, wo, chimera_group(), TAU)
    assert list(np.diff(wo.astype(np.int64))) == [37] * len(pairs)
    check_chimeras(pairs, centres, np.diff(offs.astype(np.int64)), wo, seg, ns)


# ---- placement and painting in one call, and through the driver --------------------------------------------------

def test_place_and_paint_in_one_call_equals_the_two_steps(placer_cls, case59, monkeypatch):
    data, offs = batch_for(17, 7, seed=11)
    group = groupings(59)["quarters"]
    with placer_cls.from_synth(case59) as pl:
        monkeypatch.delenv("EPIK_AMD_WINDOW_CHUNK_WINDOWS", raising=False)
        placed = pl.place_windows(data, offs, 17, 7, "both")
        want = windows.numpy_paint(placed[0], placed[1], placed[2], placed[4], group, TAU)
        assert int(want[2].max()) > 3 and (want[0]["call"] < capi.WINDOW_AMBIGUOUS).any()
        for chunk in (None, 1, 64, 65):
            if chunk is not None:
                monkeypatch.setenv("EPIK_AMD_WINDOW_CHUNK_WINDOWS", str(chunk))
            got = pl.place_and_paint_windows(data, offs, 17, 7, group, TAU, "both")
            assert same_paint(got[:5], placed) and same_paint(got[5:], want), chunk
        got = pl.place_and_paint_windows(data, offs, 17, 7, group, TAU, "both", rows_out=False)
        assert got[:3] == (None, None, None) and same_paint(got[3:5], placed[3:]) and same_paint(got[5:], want)
        with pytest.raises(capi.EpikAmdError, match=r"tau_q must lie in \(2\^29, 2\^30\]"):
            pl.place_and_paint_windows(data, offs, 17, 7, group, 1 << 29)


def test_the_driver_writes_what_python_formats(placer_cls, tmp_path):
    import os
    import subprocess
    from epik_amd import dbfile, taxonomy
    from test_profile_gpu import _write_fasta
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(200, seed=13)
    assert tree.num_nodes == CHIMERA_N
    db, refs, centres = synth.make_clade_db(CHIMERA_N, kmer_size=8, n_refs=40, ref_length=1200, width=(2.0, 0.4), seed=47)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    text = synth.synth_taxonomy(tree, 3, seed=14)
    (tmp_path / "groups.tsv").write_text(text)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    pairs = eligible_pairs(centres)[:9]
    reads = chimeras(refs, pairs)
    rc_of = str.maketrans("ACGT", "TGCA")
    reads = [r.translate(rc_of)[::-1] if i % 3 == 1 else r for i, r in enumerate(reads)]     # some arrive on the other strand
    reads += ["ACG", reads[0][:130], "N" * 200, reads[1][:119]]
    records = [(f"query {i}", s) for i, s in enumerate(reads)]
    _write_fasta(str(tmp_path / "q.fasta"), records)
    names, lengths = [n for n, _ in records], [len(s) for _, s in records]
    driver = os.path.join(root, "epik_amd", "bin", "epik-dna")
    for rank, strand, w, s in ((1, "both", CHIMERA_W, CHIMERA_S), (2, "forward", 100, 100)):
        group, group_taxa = taxonomy.groups_at_rank(taxa, label, rank)
        paths = [taxa.path[t] for t in group_taxa]
        assert len(paths) >= 2
        with placer_cls.from_synth(db, tree) as pl:
            rows, n, counts, strands, wo = pl.place_windows(*synth.pack_reads(reads), w, s, strand)
            rec, seg, ns = pl.paint_windows(rows, n, counts, wo, group, TAU)
        want = {f"windows_q.fasta.tsv": windows.format_windows_tsv(names, lengths, wo, seg, ns, paths, w, s, TAU, rank),
                f"windows_breakpoints_q.fasta.tsv": windows.format_breakpoints_tsv(names, lengths, wo, seg, ns, paths, w, s),
                f"windows_all_q.fasta.tsv": windows.format_windows_all_tsv(names, lengths, wo, rec, rows, n, strands, paths, w, s)}
        if rank == 1:
            assert want["windows_breakpoints_q.fasta.tsv"].count("\n") > 3 and "\t-\t" in want["windows_all_q.fasta.tsv"]
            assert "too_short" in want["windows_q.fasta.tsv"]
        flags = ["--windows", str(w), "--window-step", str(s), "--window-groups", str(tmp_path / "groups.tsv"), "--window-rank", str(rank),
                 "--strand", strand, "--windows-per-window"]
        for variant, extra in (("j1", ["-j", "1"]), ("j4", ["-j", "4"]), ("batch3", ["--batch-size", "3"]),
                               ("two_handles", ["--devices", "0,0", "-j", "4", "--batch-size", "2"])):
            out = tmp_path / f"out_{rank}_{variant}"
            out.mkdir()
            run = subprocess.run([driver, "-d", db_path, "-q", str(tmp_path / "q.fasta"), "-o", str(out)] + flags + extra,
                                 capture_output=True, text=True, timeout=300)
            assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
            assert sorted(p.name for p in out.iterdir()) == sorted(want), variant
            for name, content in want.items():
                assert (out / name).read_bytes() == content.encode(), (rank, variant, name)
    # without --windows-per-window: two files, the same bytes
    out = tmp_path / "out_plain"
    out.mkdir()
    run = subprocess.run([driver, "-d", db_path, "-q", str(tmp_path / "q.fasta"), "-o", str(out)] + flags[:-1], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr
    assert sorted(p.name for p in out.iterdir()) == ["windows_breakpoints_q.fasta.tsv", "windows_q.fasta.tsv"]
    assert (out / "windows_q.fasta.tsv").read_bytes() == want["windows_q.fasta.tsv"].encode()
