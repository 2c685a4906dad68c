"""Strand placement on the GPU (epik_amd_placer_place_strands[_device], Placer.place_strands, epik-dna --strand):
bit-exact against the CPU oracle run on the host-side reverse complements, the `both` rule applied to two oracle
runs, and the forward mode against the placement it wraps."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_rows_match, mixed_reads, select_kernel
from epik_amd import capi, dbfile, jplace, jplace_diff, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ["packed", "paired", "filtered", "compact", "packed-runs", "team4", "team4x3", "team2-classic",
           "team4-smallpool", "team4-block2", "paired-fewblocks", "team4-fewblocks"]

_COMP = str.maketrans("ACGTUacgtuRYKMBVDHrykmbvdhSWNswn", "TGCAAtgcaaYRMKVBHDyrmkvbhdSWNswn")


def rc(read: str) -> str:
    """The host-side reverse complement (IUPAC; other characters as they are)."""
    return read.translate(_COMP)[::-1]


def rc_packed(data, offs):
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(len(offs) - 1)]
    return synth.pack_reads([rc(r) for r in reads])


def has_rows(n):
    return (n != 0) & (n != capi.ROWS_COUNTS_TOO_NARROW)


def both_rule(fwd, rev):
    """Reverse where it has rows and either forward has none or its first score is strictly greater."""
    (fr, fn, fc), (rr, rn, rcnt) = fwd, rev
    take = has_rows(rn) & (~has_rows(fn) | (rr["score"][:, 0] > fr["score"][:, 0]))
    rows, n, counts = fr.copy(), fn.copy(), fc.copy()
    rows[take], n[take], counts[take] = rr[take], rn[take], rcnt[take]
    return (rows, n, counts), take.astype(np.uint8)


def oracle_strands(orc, data, offs):
    fwd = orc.place(data, offs, num_threads=0)
    rev = orc.place(*rc_packed(data, offs), num_threads=0)
    return fwd, rev


@pytest.fixture(params=KERNELS)
def kernel(request, monkeypatch):
    select_kernel(monkeypatch, request.param)
    return request.param


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _tricky_reads(k, rng):
    reads = mixed_reads(rng, 600, k, alphabet_amb="ACGTNRYKMSWBDHV-", max_len=200)
    reads = [r.lower() if i % 7 == 0 else r for i, r in enumerate(reads)]
    reads += ["ACGUACGUUUAC", "acgtRYKMBVDHSWN" * 3, "ACG", "", "A", "NNNNNNNNNN", "-" * 12, "AC-GTACGT-ACGT",
              "ACGTACGT", "AATTCCGGAATT", "ACGCGT" * 5]  # palindromes: a tie, forward
    return reads


def test_reverse_equals_oracle_on_reverse_complements(placer_cls, oracle_lib, small_case, kernel):
    _, db = small_case
    data, offs = synth.pack_reads(_tricky_reads(db.kmer_size, np.random.default_rng(1)))
    _, rev = oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs)
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, strand = pl.place_strands(data, offs, "reverse")
    assert_rows_match(rows, n, counts, *rev)
    assert (strand == 1).all()


def test_both_equals_the_rule_on_two_oracle_runs(placer_cls, oracle_lib, small_case, kernel):
    _, db = small_case
    reads = _tricky_reads(db.kmer_size, np.random.default_rng(2))
    pal = "ACGT" * 6                               # its own reverse complement: tie -> forward
    assert rc(pal) == pal
    reads += [pal, rc(reads[5]), rc(reads[11])]
    data, offs = synth.pack_reads(reads)
    fwd, rev = oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs)
    want, want_strand = both_rule(fwd, rev)
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, strand = pl.place_strands(data, offs, "both")
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(strand, want_strand)
    assert strand[reads.index(pal)] == 0 and strand[reads.index("")] == 0 and strand[reads.index("-" * 12)] == 0
    assert 0 < int(strand.sum()) < len(reads)


def test_forward_is_place(placer_cls, small_case, kernel):
    _, db = small_case
    data, offs = synth.pack_reads(_tricky_reads(db.kmer_size, np.random.default_rng(3)))
    with placer_cls.from_synth(db) as pl:
        want = pl.place_packed(data, offs)
        rows, n, counts, strand = pl.place_strands(data, offs, "forward")
    assert rows.tobytes() == want[0].tobytes() and n.tobytes() == want[1].tobytes()
    assert counts.tobytes() == want[2].tobytes() and not strand.any()


def test_clade_reads_flipped_come_back_reverse(placer_cls, oracle_lib, kernel):
    db, refs, _ = synth.make_clade_db(999, n_refs=80, ref_length=700, seed=5)
    data, offs = synth.make_clade_reads(refs, 1000, 150, seed=6)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(1000)]
    flipped = np.arange(1000) % 2 == 1
    mixed = [rc(r) if f else r for r, f in zip(reads, flipped)]
    mdata, moffs = synth.pack_reads(mixed)
    orc = oracle_lib.Oracle.from_synth(db)
    orig = orc.place(data, offs, num_threads=0)
    with placer_cls.from_synth(db) as pl:
        fwd_only = pl.place_packed(mdata, moffs)
        rows, n, counts, strand = pl.place_strands(mdata, moffs, "both")
    # forward alone places the flipped reads elsewhere ...
    differs = fwd_only[0]["score"][flipped, 0].view(np.uint32) != orig[0]["score"][flipped, 0].view(np.uint32)
    assert differs.mean() >= 0.95, differs.mean()
    # ... both strands find them: strand 1, the rows of the read as it was cut
    assert (strand[flipped] == 1).mean() >= 0.95, (strand[flipped] == 1).mean()
    assert not strand[~flipped].any()
    right = (strand == 1) == flipped
    assert_rows_match(rows[right], n[right], counts[right], orig[0][right], orig[1][right], orig[2][right])
    want, want_strand = both_rule(orc.place(mdata, moffs, num_threads=0), orc.place(*rc_packed(mdata, moffs), num_threads=0))
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(strand, want_strand)


def _device_run(pl, data, offs, mode, stream, ws_bytes=None):
    import torch
    dev = torch.device("cuda", pl.device)
    n, keep = len(offs) - 1, pl.keep_at_most
    d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
    d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
    d_strand = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = pl.strand_workspace_bytes(n, int(offs[-1]), mode) if ws_bytes is None else ws_bytes
    d_ws = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    pl.place_strands_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, mode, d_ws.data_ptr() if ws else 0, ws,
                            d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_strand.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return (d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(n, keep), d_n.cpu().numpy().view(np.uint32),
            d_counts.cpu().numpy().view(np.uint32).reshape(n, keep), d_strand.cpu().numpy())


def test_device_entry_on_a_side_stream(placer_cls, oracle_lib, small_case, kernel):
    import torch
    _, db = small_case
    rng = np.random.default_rng(4)
    reads = _tricky_reads(db.kmer_size, rng)[:300]
    reads += ["".join(rng.choice(list("ACGT"), size=300)) for _ in range(4)]           # 16-bit counts
    reads += ["".join(rng.choice(list("ACGTN"), size=40_000)) for _ in range(2)]       # 32-bit counts
    reads += [rc(reads[-1]), rc(reads[-3])]
    data, offs = synth.pack_reads(reads)
    fwd, rev = oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs)
    want, want_strand = both_rule(fwd, rev)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        pl.choose_counts(40_000)
        assert pl.strand_workspace_bytes(len(reads), int(offs[-1]), "forward") == 0
        assert pl.strand_workspace_bytes(len(reads), int(offs[-1]), "both") > pl.strand_workspace_bytes(
            len(reads), int(offs[-1]), "reverse") >= int(offs[-1])
        rows, n, counts, strand = _device_run(pl, data, offs, "both", stream)
        assert_rows_match(rows, n, counts, *want)
        assert np.array_equal(strand, want_strand)
        rows, n, counts, strand = _device_run(pl, data, offs, "reverse", stream)
        assert_rows_match(rows, n, counts, *rev)
        assert (strand == 1).all()
        rows, n, counts, strand = _device_run(pl, data, offs, "forward", stream)
        assert_rows_match(rows, n, counts, *fwd)
        assert not strand.any()


def test_device_entry_marks_the_same_reads_too_narrow(placer_cls, small_case, kernel):
    import torch
    _, db = small_case
    rng = np.random.default_rng(5)
    reads = mixed_reads(rng, 200, db.kmer_size, max_len=120)
    reads += ["".join(rng.choice(list("ACGT"), size=40_000)), "".join(rng.choice(list("ACGT"), size=300))]
    reads += [rc(reads[-2])]
    data, offs = synth.pack_reads(reads)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        pl.choose_counts(60)   # counts for short reads: the 40 000-letter ones do not fit
        n = len(reads)
        d_seqs = torch.from_numpy(data).cuda()
        d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
        d_rows = torch.zeros(n * pl.keep_at_most * 2, dtype=torch.float64, device="cuda")
        d_n = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(), 0,
                        stream.cuda_stream)
        stream.synchronize()
        want_n = d_n.cpu().numpy().view(np.uint32)
        rows, got_n, _, strand = _device_run(pl, data, offs, "both", stream)
    narrow = want_n == capi.ROWS_COUNTS_TOO_NARROW
    assert narrow[-1] and narrow[-3]
    assert np.array_equal(got_n == capi.ROWS_COUNTS_TOO_NARROW, narrow)
    assert not strand[narrow].any()


def test_host_entry_over_several_chunks(placer_cls, oracle_lib, small_case, monkeypatch):
    _, db = small_case
    rng = np.random.default_rng(6)
    reads = mixed_reads(rng, 2500, db.kmer_size, max_len=200)
    reads = [rc(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    reads += ["".join(rng.choice(list("ACGT"), size=40_000)), "", "ACG"]
    data, offs = synth.pack_reads(reads)
    want, want_strand = both_rule(*oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs))
    with placer_cls.from_synth(db) as pl:
        monkeypatch.setenv("EPIK_AMD_STRAND_CHUNK_READS", "333")  # eight chunks, the long read in the last
        rows, n, counts, strand = pl.place_strands(data, offs, "both")
        monkeypatch.delenv("EPIK_AMD_STRAND_CHUNK_READS")
        assert_rows_match(rows, n, counts, *want)
        assert np.array_equal(strand, want_strand)
        again = pl.place_strands(data, offs, "both")   # one chunk
        # the handle's count state is as place() leaves it: the next place() still chooses for its own batch
        short = pl.place_packed(*synth.pack_reads(reads[:50]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rows, n, counts, strand)))
    assert_rows_match(*short, *(x[:50] for x in oracle_lib.Oracle.from_synth(db).place(*synth.pack_reads(reads[:50]))))


@pytest.mark.parametrize("mode", ["forward", "reverse", "both"])
def test_host_entry_zeroes_the_slots_past_n_rows(placer_cls, oracle_lib, small_case, monkeypatch, mode):
    """Over several chunks, every row and count slot past n_rows[i] comes back zero: in `both`, also where the reverse
    strand wins with fewer rows than the forward one (its rows come from the workspace the chunk before used)."""
    _, db = small_case
    rng = np.random.default_rng(9)
    reads = mixed_reads(rng, 1500, db.kmer_size, max_len=150)
    reads = [rc(r) if i % 3 == 0 else r for i, r in enumerate(reads)]
    data, offs = synth.pack_reads(reads)
    fwd, rev = oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs)
    want = {"forward": fwd, "reverse": rev, "both": both_rule(fwd, rev)[0]}[mode]
    if mode == "both":
        take = both_rule(fwd, rev)[1].astype(bool)
        assert (take & (rev[1] < fwd[1])).any()
    with placer_cls.from_synth(db) as pl:
        keep = pl.keep_at_most
        assert keep >= 7
        monkeypatch.setenv("EPIK_AMD_STRAND_CHUNK_READS", "250")   # six chunks
        rows, n, counts, _ = pl.place_strands(data, offs, mode)
    assert_rows_match(rows, n, counts, *want)
    past = np.arange(keep)[None, :] >= n[:, None]
    assert past.any()
    assert not np.frombuffer(rows[past].tobytes(), dtype=np.uint8).any() and not counts[past].any()


@pytest.mark.parametrize("mode", ["forward", "reverse", "both"])
@pytest.mark.parametrize("forced", ["2", "0"])
def test_host_entry_widens_forced_counts_and_restores_them(placer_cls, oracle_lib, small_case, monkeypatch, forced,
                                                           mode):
    """test_parity_gpu's forced-width test for the strand host entry: a read with more k-mers than the forced width
    holds is placed, not marked; the forced width is the handle's again afterwards (the device entry marks it)."""
    import torch
    _, db = small_case
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", forced)   # 8-bit counts (255 k-mers) / 16-bit (32767)
    rng = np.random.default_rng(22)
    long_read = "".join(rng.choice(list("ACGT"), size=40_000 if forced == "0" else 700))
    data, offs = synth.pack_reads(["ACGTACGTAC", long_read, "ACGTTGCA" * 4])
    fwd, rev = oracle_strands(oracle_lib.Oracle.from_synth(db), data, offs)
    want = {"forward": fwd, "reverse": rev, "both": both_rule(fwd, rev)[0]}[mode]
    with placer_cls.from_synth(db) as pl:
        got = pl.place_strands(data, offs, mode)
        assert int(got[1].max()) <= pl.keep_at_most and capi.ROWS_COUNTS_TOO_NARROW not in got[1]
        _, dev_n, _, _ = _device_run(pl, data, offs, mode, torch.cuda.Stream())
    assert_rows_match(*got[:3], *want)
    assert dev_n[1] == capi.ROWS_COUNTS_TOO_NARROW


@pytest.mark.parametrize("keep_at_most,keep_factor", [(1, 0.01), (7, 0.01), (20, 0.01), (7, 0.3)])
def test_keep_parameters(placer_cls, oracle_lib, small_case, keep_at_most, keep_factor):
    _, db = small_case
    rng = np.random.default_rng(7)
    reads = mixed_reads(rng, 400, db.kmer_size)
    reads = [rc(r) if i % 2 else r for i, r in enumerate(reads)]
    data, offs = synth.pack_reads(reads)
    orc = oracle_lib.Oracle.from_synth(db, keep_at_most=keep_at_most, keep_factor=keep_factor)
    want, want_strand = both_rule(*oracle_strands(orc, data, offs))
    with placer_cls.from_synth(db, keep_at_most=keep_at_most, keep_factor=keep_factor) as pl:
        rows, n, counts, strand = pl.place_strands(data, offs, "both")
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(strand, want_strand)


def test_amino_handle_is_unsupported(placer_cls):
    db = synth.make_db(60, states="amino", kmer_size=3, seed=8, p_present=0.3)
    data, offs = synth.pack_reads(["ACDEFGHIKLMNPQ"])
    with placer_cls.from_synth(db) as pl:
        for mode in ("forward", "reverse", "both"):
            with pytest.raises(capi.EpikAmdError) as e:
                pl.place_strands(data, offs, mode)
            assert e.value.code == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.EpikAmdError) as e:
            pl.strand_workspace_bytes(1, 14, "both")
        assert e.value.code == capi.ERR_UNSUPPORTED


def test_place_reports_the_strand(placer_cls, small_case):
    tree, db = small_case
    with placer_cls.from_synth(db, tree) as pl:
        seq = "ACGTTGCAAGGCTTACGATCGGA"
        out = pl.place([("a", seq), ("b", rc(seq)), ("c", seq)], strand="both")
        fwd = pl.place([("a", seq)])
    assert fwd.placed_seqs[0].strand == "+"
    assert out.sequence_map[seq] == ["a", "c"]
    by_seq = {p.sequence: p for p in out.placed_seqs}
    assert {by_seq[seq].strand, by_seq[rc(seq)].strand} <= {"+", "-"}
    assert by_seq[seq].placements == fwd.placed_seqs[0].placements or by_seq[seq].strand == "-"


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for h, s in records:
            fh.write(f">{h}\n")
            for j in range(0, len(s), 70):
                fh.write(s[j:j + 70] + "\n")


@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_driver_both_strands_end_to_end(tmp_path, devices):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(500, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=80, ref_length=700, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    data, offs = synth.make_clade_reads(refs, 3000, 150, seed=15)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(3000)]
    names = [f"read_{i}" for i in range(3000)] + ["dup_fwd", "dup_rev", "short"]
    reads += [reads[2], reads[3], "ACG"]
    flipped = [i % 2 == 1 for i in range(3000)] + [False, True, False]
    fwd_fasta, mixed_fasta = str(tmp_path / "fwd.fasta"), str(tmp_path / "mixed.fasta")
    _write_fasta(fwd_fasta, list(zip(names, reads)))
    _write_fasta(mixed_fasta, [(h, rc(s) if f else s) for h, s, f in zip(names, reads, flipped)])
    out_f, out_b = tmp_path / "out_f", tmp_path / "out_b"
    out_f.mkdir(), out_b.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(out_f),
                          fwd_fasta], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert not list(out_f.glob("strands_*"))        # forward: no strands file, as before
    if devices == "0":
        cmd = [sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(out_b),
               "--strand", "both", mixed_fasta]
    else:
        cmd = [os.path.join(ROOT, "epik_amd", "bin", "epik-dna"), "-d", db_path, "-q", mixed_fasta, "-o", str(out_b),
               "--devices", devices, "--batch-size", "777", "--strand", "both"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    with open(out_b / "strands_mixed.fasta.tsv") as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert [h for h, _ in lines] == names                       # one line per record, input order
    assert {m for _, m in lines} <= {"+", "-"}
    marks = np.array([m == "-" for _, m in lines])
    fl = np.array(flipped)
    assert not marks[~fl].any()
    assert marks[fl].mean() >= 0.95, marks[fl].mean()
    got = jplace.read_jplace(str(out_b / "placements_mixed.fasta.jplace"))
    ref = jplace.read_jplace(str(out_f / "placements_fwd.fasta.jplace"))
    assert set(got) == set(ref) == set(names)
    right = [h for h, m, f in zip(names, marks, fl) if m == f]
    assert len(right) >= 0.95 * len(names)
    assert jplace_diff.diff_strict({h: got[h] for h in right}, {h: ref[h] for h in right}) == []
    assert got["short"] == []
