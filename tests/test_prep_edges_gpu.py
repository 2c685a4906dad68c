"""mate_join_kernel (with copy_forward), revcomp_kernel and translate_kernel byte for byte at their seams, and the two
selection kernels at keep = 1 and 64, on the cases of test_prep_edges_cpu.py.

The device entries (place_mates_device, place_strands_device, place_frames_device) leave the prepared sequences in the
caller's workspace.  Every case gives the entry exactly *_workspace_bytes, as a slice of a larger allocation filled with 0xA5
-- no nucleotide, residue or separator -- with 4 KiB of it on either side, runs it on a stream of its own, and then

* finds the expected bytes in the workspace: the joined sequences J_0 J_1 ..., the frames of read 0, of read 1, ..., both
  dense, and the reversed reads at the caller's own offsets; and the expected offset arrays (joined_offsets [n + 1],
  frame_offsets [m n + 1]) as uint64 bytes.  That is equality of every byte without restating the workspace's layout; a miss
  names the pair or read, the mate or frame and the first differing position (test_prep_edges_cpu.locate).  A reversed read
  or mate is compared by character class, because include/epik_amd.h defines the reverse strand by class and leaves the byte
  open (the library writes the smallest byte of the class; the host restatement keeps case); everything else by byte;
* asserts that both bands still hold 0xA5: a wrong write lands there, inside the test's own memory;
* keeps the check the other tests make: rows, n_rows, counts and the strand or frame bytes against the CPU oracle on the
  host-prepared sequences (assert_rows_match, both_rule, oracle_frames).

The batches start 0 .. 3 (mates, strands) or 0 .. 11 (frames) bytes into their buffer and have seq_offsets[0] of 0, 1, 2, 3 and
several thousand; no buffer ends where its batch ends.  What makes them reach the seams is asserted in the CPU file.
"""
import numpy as np
import pytest

import test_translate_gpu
from conftest import assert_rows_match, select_kernel
from epik_amd import mates, synth
from test_prep_edges_cpu import (BAND, BATCH_SIZES, EDGE_KEEPS, FILL, FRAME_CASES, MATES_CASES, STRAND_CASES, _latin, amino_db,
                                 assert_occurs, cached_frames, frame_batch, frames_pattern, joined_offsets, joined_pattern,
                                 joined_sequences, mates_bad_batch, mates_batch, nucl_db, offsets_pattern, reversed_pattern,
                                 selection_kinds, selection_reads, selection_reference, selection_singles, strand_batch)
from test_strand_cpu import rc
from test_strand_gpu import both_rule
from test_translate_gpu import oracle_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _run(pl, batch, n, ws_bytes, stream, call):
    """The entry on `stream` with a workspace of exactly ws_bytes between two bands of FILL.  Returns (rows, n_rows, counts,
    label) and the workspace as the entry left it."""
    import torch
    from epik_amd import capi
    dev = torch.device("cuda", pl.device)
    keep = pl.keep_at_most
    d_buffer = torch.from_numpy(batch.buffer).to(dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(batch.offsets).view(np.int64)).to(dev)
    arena = torch.full((BAND + ws_bytes + BAND,), FILL, dtype=torch.uint8, device=dev)
    # (the low bits of every source and destination address are then those of the offsets, as the CPU file counts them)
    assert d_buffer.data_ptr() % 256 == 0 and arena.data_ptr() % 256 == 0 and ws_bytes % 8 == 0 and ws_bytes > 0
    d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
    d_label = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    call(d_buffer.data_ptr() + batch.lead, d_offs.data_ptr(), arena.data_ptr() + BAND, d_rows.data_ptr(), d_n.data_ptr(),
         d_counts.data_ptr(), d_label.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    host = arena.cpu().numpy()
    for name, band in (("in front of", host[:BAND]), ("behind", host[BAND + ws_bytes:])):
        touched = np.nonzero(band != FILL)[0]
        assert touched.size == 0, f"{batch.name}: the band {name} the workspace was written, first at its byte {int(touched[0])}"
    got = (d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(n, keep), d_n.cpu().numpy().view(np.uint32),
           d_counts.cpu().numpy().view(np.uint32).reshape(n, keep), d_label.cpu().numpy())
    return got, host[BAND:BAND + ws_bytes]


def _assert_strand_result(got, strand, fwd, rev, what):
    rows, n, counts, label = got
    if strand == "both":
        want, want_label = both_rule(fwd, rev)
    else:
        want, want_label = (fwd, np.zeros(len(n), np.uint8)) if strand == "forward" else (rev, np.ones(len(n), np.uint8))
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(label, want_label), what


# ---- mates --------------------------------------------------------------------------------------------------------------
def _check_mates(pl, orc, batch, orientation, strand, sep, stream, bad=()):
    n = len(batch.reads) // 2
    seq_bytes = int(batch.offsets[-1]) - batch.base
    what = f"{batch.name}, {orientation}, {strand}"
    pl.choose_counts(max(len(batch.reads[2 * i]) + len(batch.reads[2 * i + 1]) + 1 for i in range(n)))
    ws_bytes = pl.mates_workspace_bytes(n, seq_bytes, strand, orientation)
    got, ws = _run(pl, batch, n, ws_bytes, stream,
                   lambda seqs, offs, d_ws, *out: pl.place_mates_device(seqs, offs, n, seq_bytes, strand, orientation, d_ws, ws_bytes, *out))
    assert_occurs(ws, joined_pattern(batch, orientation, sep, bad), f"the joined sequences ({what})")
    assert_occurs(ws, offsets_pattern(joined_offsets(batch), "joined_offsets"), f"the joined offsets ({what})")
    joined = [j for j, _ in joined_sequences(batch, orientation, sep, bad)]
    if strand != "forward":
        # (the range of a pair left unjoined holds FILL; reversed, the library's byte for an invalid character)
        names = [f"{batch.name}: J of pair {i}" for i in range(n)]
        assert_occurs(ws, reversed_pattern([j.replace(bytes([FILL]), b"-") for j in joined], names), f"the reversed joined sequences ({what})")
    fwd = orc.place(*synth.pack_reads(joined), num_threads=0)
    rev = orc.place(*synth.pack_reads([rc(j) for j in joined]), num_threads=0) if strand != "forward" else None
    _assert_strand_result(got, strand, fwd, rev, what)


@pytest.mark.parametrize("strand", ["forward", "reverse", "both"])
@pytest.mark.parametrize("orientation", ["fr", "ff"])
def test_mate_join_writes_every_byte_at_every_alignment(placer_cls, oracle_lib, small_case, monkeypatch, orientation, strand):
    import torch
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    orc = oracle_lib.Oracle.from_synth(db)
    stream = torch.cuda.Stream()
    assert {case[0] for case in MATES_CASES} == set(BATCH_SIZES)
    with placer_cls.from_synth(db) as pl:
        sep = pl.mates_separator()
        assert sep == ord("-")
        for case in MATES_CASES:
            _check_mates(pl, orc, mates_batch(*case), orientation, strand, sep, stream)


@pytest.mark.parametrize("orientation,strand", [("fr", "both"), ("ff", "forward")])
def test_mate_join_leaves_pairs_with_offsets_out_of_order_alone(placer_cls, oracle_lib, small_case, monkeypatch, orientation, strand):
    """Two pairs (m < b, e < m) between good ones: the good pairs' bytes and every joined offset as specified, the bad pairs'
    ranges still 0xA5, the bands untouched."""
    import torch
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    batch, bad = mates_bad_batch()
    with placer_cls.from_synth(db) as pl:
        _check_mates(pl, oracle_lib.Oracle.from_synth(db), batch, orientation, strand, pl.mates_separator(), torch.cuda.Stream(), bad)


# ---- strands ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reverse", "both"])
def test_revcomp_writes_every_byte_at_the_callers_offsets(placer_cls, oracle_lib, small_case, monkeypatch, mode):
    import torch
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    orc = oracle_lib.Oracle.from_synth(db)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        for case in STRAND_CASES:
            batch = strand_batch(*case)
            n, what = len(batch.reads), f"{batch.name}, {mode}"
            pl.choose_counts(max(len(r) for r in batch.reads))
            ws_bytes = pl.strand_workspace_bytes(n, int(batch.offsets[-1]), mode)       # (sized by seq_offsets[n], as the header says)
            got, ws = _run(pl, batch, n, ws_bytes, stream,
                           lambda seqs, offs, d_ws, *out: pl.place_strands_device(seqs, offs, n, mode, d_ws, ws_bytes, *out))
            names = [f"{batch.name}: read {i}" for i in range(n)]
            assert_occurs(ws, reversed_pattern(batch.reads, names, lead_fill=min(batch.base, 64)), f"the reversed reads ({what})")
            fwd = orc.place(*synth.pack_reads(batch.reads), num_threads=0)
            rev = orc.place(*synth.pack_reads([rc(r) for r in batch.reads]), num_threads=0)
            _assert_strand_result(got, mode, fwd, rev, what)


# ---- frames -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["forward", "reverse", "both"])
def test_translate_writes_every_residue_at_every_shift_and_seam(placer_cls, oracle_lib, monkeypatch, mode):
    import torch
    select_kernel(monkeypatch, "packed")
    # (oracle_frames translates through this name: the same frames, computed once a read)
    monkeypatch.setattr(test_translate_gpu, "frames", cached_frames)
    db = amino_db()
    orc = oracle_lib.Oracle.from_synth(db)
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        for name in FRAME_CASES:
            batch = frame_batch(name)
            n, what = len(batch.reads), f"{batch.name}, {mode}"
            pl.choose_counts(max(len(r) for r in batch.reads) // 3)
            ws_bytes = pl.frame_workspace_bytes(n, int(batch.offsets[-1]), mode)
            got, ws = _run(pl, batch, n, ws_bytes, stream,
                           lambda seqs, offs, d_ws, *out: pl.place_frames_device(seqs, offs, n, mode, d_ws, ws_bytes, *out))
            pattern, offsets = frames_pattern(batch, mode)
            assert_occurs(ws, pattern, f"the frames ({what})")
            assert_occurs(ws, offsets_pattern(offsets, "frame_offsets"), f"the frame offsets ({what})")
            want, want_frame = oracle_frames(orc, [_latin(r) for r in batch.reads], mode, db.kmer_size, pl.keep_at_most)
            rows, n_rows, counts, frame = got
            assert_rows_match(rows, n_rows, counts, *want)
            assert np.array_equal(frame, want_frame), what


# ---- the selection kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep,factor", EDGE_KEEPS)
@pytest.mark.parametrize("kind", ["strands", "mates", "frames"])
def test_selection_kernels_at_keep_1_and_64(placer_cls, oracle_lib, monkeypatch, kind, keep, factor):
    """strand_select_kernel and frame_select_kernel divide slot indices by keep: batches of 1, 63, 64, 65 and 257 reads or pairs
    through the host entries, every row against the oracle's rule, every slot past n_rows zero."""
    select_kernel(monkeypatch, "packed")
    monkeypatch.setattr(test_translate_gpu, "frames", cached_frames)
    want, label = selection_reference(oracle_lib, kind, keep, factor)
    reads = selection_reads(kind)
    batches = [list(range(n)) for n in BATCH_SIZES[1:]] + [[i] for i in selection_singles(selection_kinds(label, want[1]))]
    assert sorted({len(b) for b in batches}) == sorted(BATCH_SIZES)
    with placer_cls.from_synth(amino_db() if kind == "frames" else nucl_db(), keep_at_most=keep, keep_factor=factor) as pl:
        assert pl.keep_at_most == keep
        for index in batches:
            if kind == "mates":
                got = pl.place_mates(*mates.interleave([reads[2 * i] for i in index], [reads[2 * i + 1] for i in index]), "both")
            elif kind == "strands":
                got = pl.place_strands(*synth.pack_reads([reads[i] for i in index]), "both")
            else:
                got = pl.place_frames(*synth.pack_reads([reads[i] for i in index]), "both")
            rows, n_rows, counts, got_label = got
            assert_rows_match(rows, n_rows, counts, *(a[index] for a in want))
            assert np.array_equal(got_label, label[index]), (kind, keep, len(index))
            past = np.arange(keep)[None, :] >= n_rows[:, None]
            assert not np.frombuffer(rows[past].tobytes(), dtype=np.uint8).any() and not counts[past].any(), (kind, keep, len(index))
