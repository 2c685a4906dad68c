"""Translated placement on the GPU (epik_amd_placer_place_frames[_device], Placer.place_frames, epik-aa --translate):
bit-exact against the CPU oracle run on host-translated frames (test_translate_cpu's translation, built from the
64 codons written out), with the frame rule applied on the host to the oracle's m results per read."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_rows_match, select_kernel
from epik_amd import alphabet, capi, dbfile, jplace, jplace_diff, synth
from test_translate_cpu import STANDARD_CODE, frames, revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel variants of test_strand_gpu.py that apply to a protein database (the paired layout is nucleotide-only)
KERNELS = ["packed", "filtered", "compact", "packed-runs", "team4", "team4x3", "team2-classic", "team4-smallpool",
           "team4-block2", "packed-fewblocks", "team4-fewblocks"]
MODES = ["forward", "reverse", "both"]


def has_rows(n):
    return (n != 0) & (n != capi.ROWS_COUNTS_TOO_NARROW)


def oracle_frames(orc, reads, mode, k, keep):
    """The oracle on the host-translated frames of every read, and the frame rule applied to its m results per
    read: (rows, n_rows, counts), frame bytes."""
    m = 6 if mode == "both" else 3
    first = 3 if mode == "reverse" else 0
    fr = [f for r in reads for f in frames(r, mode)]
    data, offs = synth.pack_reads(fr)
    rows, n_rows, counts = orc.place(data, offs, num_threads=0)
    n = len(reads)
    lens = np.array([len(f) for f in fr], dtype=np.int64).reshape(n, m)
    rows, n_rows, counts = rows.reshape(n, m, keep), n_rows.reshape(n, m), counts.reshape(n, m, keep)
    out_rows = np.zeros((n, keep), dtype=capi.PLACEMENT)
    out_n = np.zeros(n, dtype=np.uint32)
    out_c = np.zeros((n, keep), dtype=np.uint32)
    out_f = np.full(n, first, dtype=np.uint8)
    for i in range(n):
        if (n_rows[i] == capi.ROWS_COUNTS_TOO_NARROW).any():
            out_n[i] = capi.ROWS_COUNTS_TOO_NARROW
            continue
        best, best_key = -1, None
        for w in range(m):
            if not has_rows(n_rows[i, w]):
                continue
            key = np.float32(rows[i, w, 0]["score"]) / np.float32(lens[i, w] - k + 1)
            if best < 0 or key > best_key:
                best, best_key = w, key
        if best < 0:
            out_n[i] = n_rows[i, 0]
            continue
        out_rows[i], out_n[i], out_c[i], out_f[i] = rows[i, best], n_rows[i, best], counts[i, best], first + best
    return (out_rows, out_n, out_c), out_f


@pytest.fixture(params=KERNELS)
def kernel(request, monkeypatch):
    select_kernel(monkeypatch, request.param)
    return request.param


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


@pytest.fixture(scope="module")
def amino_small():
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    return tree, db


def _tricky_reads(rng, n=300):
    reads = []
    for i in range(n):
        alpha = "ACGT" if i % 3 else "ACGTUNRYKMSWBDHV-."
        read = "".join(rng.choice(list(alpha), size=int(rng.integers(0, 200))))
        reads.append(read.lower() if i % 7 == 0 else read)
    reads += ["", "A", "AC", "ACG", "ACGT", "ACGTA",             # lengths 0..5
              "TAATAGTGATAATAGTGA", "ATGTAAATGTAGATGTGA" * 3,    # stops
              "atgaaaCCCgggtttUUU" * 4, "ACG-TAC.GTA*CGTNNNRYA" * 4, "NNNNNNNNNNNN", "-" * 15]
    return reads


def back_translate(protein: str, rng) -> str:
    codons = {}
    for codon, aa in STANDARD_CODE.items():
        codons.setdefault(aa, []).append(codon)
    return "".join(codons[a][int(rng.integers(0, len(codons[a])))] for a in protein)


@pytest.mark.parametrize("mode", MODES)
def test_modes_equal_the_oracle_on_host_translated_frames(placer_cls, oracle_lib, amino_small, kernel, mode):
    _, db = amino_small
    reads = _tricky_reads(np.random.default_rng(1))
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db)
    with placer_cls.from_synth(db) as pl:
        want, want_frame = oracle_frames(orc, reads, mode, db.kmer_size, pl.keep_at_most)
        rows, n, counts, frame = pl.place_frames(data, offs, mode)
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(frame, want_frame)
    assert has_rows(n).mean() > 0.5


def test_large_tree_team_path(placer_cls, oracle_lib, monkeypatch):
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    tree = synth.make_tree(2000, seed=30)                    # N = 3 999: create() chooses the team placement
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=31, p_present=0.3)
    reads = _tricky_reads(np.random.default_rng(2), 400)
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db)
    with placer_cls.from_synth(db) as pl:
        want, want_frame = oracle_frames(orc, reads, "both", db.kmer_size, pl.keep_at_most)
        rows, n, counts, frame = pl.place_frames(data, offs, "both")
        assert pl.last_path() != capi.PATH_WAVE
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(frame, want_frame)


def _device_run(pl, data, offs, mode, stream):
    import torch
    dev = torch.device("cuda", pl.device)
    n, keep = len(offs) - 1, pl.keep_at_most
    d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
    d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
    d_frame = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = pl.frame_workspace_bytes(n, int(offs[-1]), mode)
    d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pl.place_frames_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, mode, d_ws.data_ptr(), ws, d_rows.data_ptr(),
                           d_n.data_ptr(), d_counts.data_ptr(), d_frame.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return (d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(n, keep), d_n.cpu().numpy().view(np.uint32),
            d_counts.cpu().numpy().view(np.uint32).reshape(n, keep), d_frame.cpu().numpy())


def test_device_entry_on_a_side_stream(placer_cls, oracle_lib, amino_small, kernel):
    import torch
    _, db = amino_small
    rng = np.random.default_rng(4)
    reads = _tricky_reads(rng, 200)
    reads += ["".join(rng.choice(list("ACGT"), size=1200)) for _ in range(3)]        # 16-bit counts
    reads += ["".join(rng.choice(list("ACGTN"), size=3000)), revcomp(reads[-1])]    # windows of several tiles
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        pl.choose_counts(1000)
        for mode in MODES:
            want, want_frame = oracle_frames(orc, reads, mode, db.kmer_size, pl.keep_at_most)
            rows, n, counts, frame = _device_run(pl, data, offs, mode, stream)
            assert_rows_match(rows, n, counts, *want)
            assert np.array_equal(frame, want_frame)


def test_device_entry_too_narrow_agrees_with_the_frames(placer_cls, amino_small):
    """TOO_NARROW: a read is marked exactly when place_device marks one of its frames."""
    import torch
    _, db = amino_small
    rng = np.random.default_rng(15)
    reads = _tricky_reads(rng, 60) + ["".join(rng.choice(list("ACGT"), size=2400)),
                                       "".join(rng.choice(list("ACGT"), size=900))]
    data, offs = synth.pack_reads(reads)
    fr = [f for r in reads for f in frames(r, "both")]
    fdata, foffs = synth.pack_reads(fr)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        capi.check(pl._lib.epik_amd_placer_set_wide_counts(pl._handle, 2))   # 8-bit counts: frames of more than 255 k-mers do not fit
        nf = len(fr)
        d_seqs = torch.from_numpy(fdata).cuda()
        d_offs = torch.from_numpy(foffs.view(np.int64)).cuda()
        d_rows = torch.zeros(nf * pl.keep_at_most * 2, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(nf, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), nf, d_rows.data_ptr(), d_n.data_ptr(), 0,
                        stream.cuda_stream)
        stream.synchronize()
        frame_narrow = (d_n.cpu().numpy().view(np.uint32) == capi.ROWS_COUNTS_TOO_NARROW).reshape(len(reads), 6)
        _, got_n, _, _ = _device_run(pl, data, offs, "both", stream)
    assert frame_narrow[-1].any() and frame_narrow[-2].any()
    assert np.array_equal(got_n == capi.ROWS_COUNTS_TOO_NARROW, frame_narrow.any(axis=1))


def test_host_entry_over_several_chunks(placer_cls, oracle_lib, amino_small, monkeypatch):
    _, db = amino_small
    rng = np.random.default_rng(6)
    reads = _tricky_reads(rng, 1500) + ["".join(rng.choice(list("ACGT"), size=3000)), "", "AC"]
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db)
    with placer_cls.from_synth(db) as pl:
        want, want_frame = oracle_frames(orc, reads, "both", db.kmer_size, pl.keep_at_most)
        monkeypatch.setenv("EPIK_AMD_FRAME_CHUNK_READS", "333")   # five chunks
        rows, n, counts, frame = pl.place_frames(data, offs, "both")
        monkeypatch.delenv("EPIK_AMD_FRAME_CHUNK_READS")
        again = pl.place_frames(data, offs, "both")              # one chunk
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(frame, want_frame)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rows, n, counts, frame)))


@pytest.mark.parametrize("mode", MODES)
def test_host_entry_zeroes_the_slots_past_n_rows(placer_cls, oracle_lib, amino_small, monkeypatch, mode):
    """Over several chunks, every row and count slot past n_rows[i] comes back zero, also where the winning frame has
    fewer rows than a losing one."""
    _, db = amino_small
    reads = _tricky_reads(np.random.default_rng(16), 1500)
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db)
    per_frame = orc.place(*synth.pack_reads([f for r in reads for f in frames(r, mode)]), num_threads=0)[1]
    with placer_cls.from_synth(db) as pl:
        keep = pl.keep_at_most
        assert keep >= 7
        want, _ = oracle_frames(orc, reads, mode, db.kmer_size, keep)
        assert (has_rows(want[1]) & (want[1] < per_frame.reshape(len(reads), -1).max(axis=1))).any()
        monkeypatch.setenv("EPIK_AMD_FRAME_CHUNK_READS", "333")   # five chunks
        rows, n, counts, _ = pl.place_frames(data, offs, mode)
    assert_rows_match(rows, n, counts, *want)
    past = np.arange(keep)[None, :] >= n[:, None]
    assert past.any()
    assert not np.frombuffer(rows[past].tobytes(), dtype=np.uint8).any() and not counts[past].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("forced", ["2", "0"])
def test_host_entry_widens_forced_counts_and_restores_them(placer_cls, oracle_lib, amino_small, monkeypatch, forced,
                                                           mode):
    """test_parity_gpu's forced-width test for the frame host entry: a frame with more k-mers than the forced width
    holds is placed, not marked; the forced width is the handle's again afterwards (the device entry marks it)."""
    import torch
    _, db = amino_small
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", forced)   # 8-bit counts (255 k-mers) / 16-bit (32767)
    rng = np.random.default_rng(23)
    long_read = "".join(rng.choice(list("ACGT"), size=100_000 if forced == "0" else 900))
    reads = ["ACGTACGTACGTACGT", long_read, "ATGGCTAAACGTGATGAACTTCAGGGTCCG"]
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl:
        want, want_frame = oracle_frames(oracle_lib.Oracle.from_synth(db), reads, mode, db.kmer_size, pl.keep_at_most)
        got = pl.place_frames(data, offs, mode)
        assert int(got[1].max()) <= pl.keep_at_most and capi.ROWS_COUNTS_TOO_NARROW not in got[1]
        _, dev_n, _, _ = _device_run(pl, data, offs, mode, torch.cuda.Stream())
    assert_rows_match(*got[:3], *want)
    assert np.array_equal(got[3], want_frame)
    assert dev_n[1] == capi.ROWS_COUNTS_TOO_NARROW


def test_nucleotide_handle_is_refused(placer_cls, small_case):
    _, db = small_case
    data, offs = synth.pack_reads(["ACGTACGTACGT"])
    with placer_cls.from_synth(db) as pl:
        for mode in MODES:
            with pytest.raises(capi.EpikAmdError) as e:
                pl.place_frames(data, offs, mode)
            assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.EpikAmdError) as e:
            pl.frame_workspace_bytes(1, 12, "both")
        assert e.value.code == capi.ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def amino_sparse():
    tree = synth.make_tree(200, seed=40)
    # (few present k-mers, so that a noise frame rarely hits one; long lists, so that the planted k-mers of a read
    # share branches)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=5, seed=41, p_present=0.001, lognormal=(4.5, 0.3))
    return tree, db


def test_back_translated_reads_come_back_in_their_frame(placer_cls, oracle_lib, amino_sparse):
    _, db = amino_sparse
    pdata, poffs = synth.reads_hitting(db, 1000, 50, hit_rate=1.0, seed=42)
    proteins = [bytes(pdata[int(poffs[i]):int(poffs[i + 1])]).decode() for i in range(1000)]
    rng = np.random.default_rng(43)
    flipped = np.arange(1000) % 2 == 1
    reads = [back_translate(p, rng) for p in proteins]
    reads = [revcomp(r) if f else r for r, f in zip(reads, flipped)]
    assert all(frames(r, "reverse" if f else "forward")[0] == p for r, f, p in zip(reads, flipped, proteins))
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, frame = pl.place_frames(data, offs, "both")
        want, want_frame = oracle_frames(oracle_lib.Oracle.from_synth(db), reads, "both", db.kmer_size, pl.keep_at_most)
        direct = pl.place_packed(pdata, poffs)
    generating = np.where(flipped, 3, 0)
    assert (frame == generating).mean() >= 0.95, (frame == generating).mean()
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(frame, want_frame)
    right = frame == generating                       # those are placed as their protein is
    assert_rows_match(rows[right], n[right], counts[right], direct[0][right], direct[1][right], direct[2][right])


def test_place_reports_the_frame(placer_cls, amino_small):
    tree, db = amino_small
    with placer_cls.from_synth(db, tree) as pl:
        seq = "ATGGCTAAACGTGATGAACTTCAGGGTCCG"
        out = pl.place([("a", seq), ("b", revcomp(seq)), ("c", seq)], translate="both")
        plain = pl.place([("a", "MAKRDELQGP")])
        with pytest.raises(ValueError):
            pl.place([("a", seq)], translate="sideways")
    assert plain.placed_seqs[0].frame == ""
    assert out.sequence_map[seq] == ["a", "c"]
    assert {p.frame for p in out.placed_seqs} <= set(capi.FRAME_NAMES)


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for h, s in records:
            fh.write(f">{h}\n")
            for j in range(0, len(s), 70):
                fh.write(s[j:j + 70] + "\n")


def test_launcher_translate_both_end_to_end(tmp_path, oracle_lib, amino_sparse):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree, db = amino_sparse
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    pdata, poffs = synth.reads_hitting(db, 1500, 50, hit_rate=1.0, seed=50)
    rng = np.random.default_rng(51)
    reads = [back_translate(bytes(pdata[int(poffs[i]):int(poffs[i + 1])]).decode(), rng) for i in range(1500)]
    reads = [revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
    reads += [reads[0], reads[1], "ACG", "NNNNNNNNNNNNNNNNNNNNNNNN"]
    names = [f"read_{i}" for i in range(len(reads))]
    query = str(tmp_path / "nt.fasta")
    _write_fasta(query, list(zip(names, reads)))
    out = tmp_path / "out"
    out.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-s", "amino", "-i", db_path, "-o",
                          str(out), "--translate", "both", query], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    # the expectation: the oracle on the host-translated frames, the rule on the host; the winning frames' protein
    # reads placed as such (epik-aa without --translate) give the jplace rows
    orc = oracle_lib.Oracle.from_synth(db)
    _, want_frame = oracle_frames(orc, reads, "both", db.kmer_size, 7)
    with open(out / "frames_nt.fasta.tsv") as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert [h for h, _ in lines] == names
    assert [f for _, f in lines] == [capi.FRAME_NAMES[int(f)] for f in want_frame]
    proteins = [frames(r, "both")[int(f)] for r, f in zip(reads, want_frame)]
    pquery = str(tmp_path / "aa.fasta")
    _write_fasta(pquery, list(zip(names, proteins)))
    out_p = tmp_path / "out_p"
    out_p.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-s", "amino", "-i", db_path, "-o",
                          str(out_p), pquery], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert not list(out_p.glob("frames_*"))
    got = jplace.read_jplace(str(out / "placements_nt.fasta.jplace"))
    ref = jplace.read_jplace(str(out_p / "placements_aa.fasta.jplace"))
    assert set(got) == set(ref) == set(names)
    assert jplace_diff.diff_strict(got, ref) == []
    assert got[names[-2]] == []
    assert alphabet.char_class_table("amino")[ord("*")] == 0
