"""The cases that take mate_join_kernel (with copy_forward), revcomp_kernel, translate_kernel and the two selection kernels to
their seams, the bytes they have to write, and what keeps the GPU sweep of test_prep_edges_gpu.py from passing vacuously.

The three kernels that rewrite the reads in front of the placement were checked only through the rows that come out behind
them, on reads of ordinary length at offset 0 of a fresh allocation.  A wrong byte at a seam -- the head, the funnel-shifted
dwords or the tail of copy_forward at one of the 16 pairs of source and destination alignment, the 1 024- and 256-byte passes,
one of the 16 load shifts of a translation window, the two bytes of lookahead behind its 768 codon starts, a reverse run
indexed from T - t1, a batch whose seq_offsets[0] is not 0 -- had to change a kept row of a random database to be seen.

Here the expected bytes are built on the host with the restatements the CPU tests already hold (mates.join,
test_strand_cpu.rc, test_translate_cpu.frames); the GPU file finds them in the workspace the device entries leave behind,
byte for byte.  Where the library's complement map leaves the byte open (include/epik_amd.h defines the reverse strand by
character CLASS: the library writes the smallest byte of the complemented class, the host restatements keep case and the
invalid byte), a position is compared by class: that is every position of a reversed read or mate, and no other.

This file asserts, on the host alone: every (source & 3, destination & 3) pair of copy_forward occurs for copies of a dword
and more; every (load shift, L mod 3) pair occurs at every window seam; the expected frames hold all 20 residues and B Z J X *;
the codons over the window seams carry ambiguous codes, lower case, U, an invalid byte and stops in both directions; every
selection batch has reads where the reverse strand or a later frame wins, where the forward strand or the first frame wins,
and reads without rows; and that `locate` names the pair, the part and the position of a wrong byte.
"""
import bisect
import contextlib
import functools
from dataclasses import dataclass, field

import numpy as np
import pytest

import test_translate_cpu
from epik_amd import alphabet, capi, mates, synth
from test_strand_cpu import bitrev4, rc
from test_translate_cpu import frames

FILL = 0xA5                     # no nucleotide, residue or separator: what the workspace and the bands hold beforehand
BAND = 4096                     # bytes of FILL on either side of the workspace
PAD = 256                       # bytes behind a batch in its buffer (no buffer ends where its batch ends)
BATCH_SIZES = (1, 63, 64, 65, 257)     # one, a partial and a full group of 64, one more, more than a workgroup's 256
MATE_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1031)
STRAND_LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
K_TILE = 768                    # frame_place.hip: codon starts a window
FRAME_SEAMS = {1: (769, 770, 771), 2: (1537, 1538, 1539, 1540), 3: (2305, 2306, 2307)}    # T = L - 2 around 768, 1 536, 2 304
FRAME_LONG = tuple(L for group in FRAME_SEAMS.values() for L in group)
SEAM_POSITIONS = (tuple(range(766, 771)), tuple(range(1534, 1539)))
RESIDUES = set("ACDEFGHIKLMNPQRSTVWY") | set("BZJX*")
EDGE_KEEPS = ((1, 0.0), (64, 0.01))

RICH = b"ACGTUacgtuRYKMSWBDHVNrykmswbdhvn-.*X\xff"       # IUPAC codes, lower case, U, invalid bytes
# nine bytes over a window seam (nucleotides 764 .. 772, moved by 0, 1 or 2): RAY SAR MTH are B Z J, stops forward (TAA TAG TGA)
# and reverse (TTA CTA TCA), ambiguous codes, lower case, U and invalid bytes next to them
MOTIFS = (b"RAYSARMTH", b"TAAryNuGA", b"c-TGAUUrY", b"TTAtcaCTA", b"NNNACGugc", b"aYgKtMcSw", b"DTAGHVBgU", b".AtGuAAyR",
          b"\xffTAGcTAat")

NUCL_CLASS = alphabet.char_class_table("nucl").astype(np.uint8)
assert NUCL_CLASS[FILL] == 0 and FILL not in RICH and FILL not in b"".join(MOTIFS)
# the view a class comparison is made in: a byte's class, the FILL byte apart (the library writes the smallest byte of class 0
# for an invalid character, never FILL)
VIEW = NUCL_CLASS.copy()
VIEW[FILL] = FILL
assert int(NUCL_CLASS.max()) <= 15
BITREV = np.array([bitrev4(c) for c in range(16)], dtype=np.uint8)


# ---- batches: what the device buffer holds, where the batch starts in it, its offsets -------------------------------
@dataclass
class Batch:
    """`buffer` is uploaded whole to a 256-byte-aligned allocation; d_seqs = its address + lead; offsets[0] = the base."""
    buffer: np.ndarray
    lead: int
    offsets: np.ndarray
    reads: list
    name: str = ""

    @property
    def base(self):
        return int(self.offsets[0])

    def address(self, i):
        """The device address of read i's first byte, relative to the allocation (its low 8 bits are the address's own)."""
        return self.lead + int(self.offsets[i])


def _noise(rng, size):
    return bytes(rng.choice(list(b"ACGT"), size=size).astype(np.uint8))


def random_read(rng, length, rich=0.1):
    plain = rng.choice(list(b"ACGT"), size=length)
    other = rng.choice(list(RICH), size=length)
    return bytes(np.where(rng.random(length) < rich, other, plain).astype(np.uint8))


def make_batch(reads, lead=0, base=0, seed=0, name=""):
    rng = np.random.default_rng(seed + 977)
    offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
    offsets += np.uint64(base)
    buffer = np.frombuffer(_noise(rng, lead + base) + b"".join(reads) + _noise(rng, PAD), dtype=np.uint8).copy()
    return Batch(buffer, lead, offsets, list(reads), name or f"n = {len(reads)}, lead {lead}, base {base}")


# ---- patterns: the bytes to find, which of them by class, and what lies where ---------------------------------------
@dataclass
class Pattern:
    exact: np.ndarray                      # the expected bytes (at an open position: a byte of the expected class)
    closed: np.ndarray = None              # False where the byte is open and the class is compared; None: every byte counts
    segments: list = field(default_factory=list)   # (start, label), ascending

    def describe(self, pos):
        if not self.segments:
            return f"position {pos}"
        i = max(bisect.bisect_right([s for s, _ in self.segments], pos) - 1, 0)
        return f"{self.segments[i][1]}, position {pos - self.segments[i][0]} of it (byte {pos} of the expected string)"


def locate(ws, pattern, what):
    """(where `pattern` occurs in the uint8 array `ws`, None), or (-1, a message that names the first differing position)."""
    ws = np.ascontiguousarray(ws, dtype=np.uint8)
    exact = np.ascontiguousarray(pattern.exact, dtype=np.uint8)
    by_class = pattern.closed is not None
    hay, needle = (VIEW[ws].tobytes(), VIEW[exact].tobytes()) if by_class else (ws.tobytes(), exact.tobytes())
    at, differs = hay.find(needle), None
    while at >= 0:
        if not by_class:
            return at, None
        bad = np.nonzero(pattern.closed & (ws[at:at + exact.size] != exact))[0]
        if bad.size == 0:
            return at, None
        differs = differs or (at, int(bad[0]))
        at = hay.find(needle, at + 1)
    if differs:
        at, j = differs
        return -1, (f"{what}: the classes are found at byte {at} of the workspace, but {pattern.describe(j)} is {int(ws[at + j]):#04x}, "
                    f"expected {int(exact[j]):#04x}")
    # Where the string should lie: where its longest prefix that occurs anywhere does, or where its longest suffix puts its
    # first byte -- whichever leaves fewer bytes different; the first of those is named.
    def longest(part):
        lo, hi = 0, len(needle) + 1          # a part of lo bytes occurs, one of hi bytes does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if hay.find(part(mid)) >= 0 else (lo, mid)
        return lo
    head, tail = longest(lambda m: needle[:m]), longest(lambda m: needle[len(needle) - m:])
    starts = {hay.find(needle[:head]), hay.find(needle[len(needle) - tail:]) - (len(needle) - tail)}
    view, want = np.frombuffer(hay, dtype=np.uint8), np.frombuffer(needle, dtype=np.uint8)
    best = None
    for start in sorted(s for s in starts if 0 <= s <= len(hay) - len(needle)):
        wrong = np.nonzero(view[start:start + len(needle)] != want)[0]
        if best is None or wrong.size < best[1].size:
            best = (start, wrong)
    if best is None:
        return -1, f"{what}: not in the workspace, and no place in it holds the string's first {head} or last {tail} bytes whole"
    start, wrong = best
    j = int(wrong[0])
    return -1, (f"{what}: not in the workspace; laid over byte {start} of it, {wrong.size} of {len(needle)} bytes differ, the first of them "
                f"{pattern.describe(j)}: {int(view[start + j]):#04x}, expected {int(want[j]):#04x}" + (" (classes)" if by_class else ""))


def assert_occurs(ws, pattern, what):
    at, message = locate(ws, pattern, what)
    assert message is None, message
    return at


def offsets_pattern(values, name):
    exact = np.asarray(values, dtype="<u8").view(np.uint8)
    return Pattern(exact, None, [(8 * i, f"{name}[{i}] = {int(v)}") for i, v in enumerate(values)])


# ---- mates --------------------------------------------------------------------------------------------------------------
# (pairs, lead, base): every batch size at base 0, a batch 1, 2 and 3 bytes into its buffer, bases 1, 2, 3 and several thousand
MATES_CASES = ((1, 0, 0), (63, 1, 0), (64, 2, 0), (65, 3, 0), (257, 0, 0), (64, 0, 1), (65, 0, 2), (63, 0, 3), (64, 1, 4099),
               (65, 2, 5003), (257, 3, 2))
MATES_SPECIAL = ((0, 0), (0, 1031), (1025, 0), (0, 5), (3, 0))     # both mates empty, one empty on either side


def mates_lengths(n):
    """Pair i: mate 1 walks through MATE_LENGTHS, mate 2 through them in steps of 7 (every 18 pairs: every length on either
    side); the first pairs are the empty ones.  One pair alone: 1 025 and 1 031, past a 1 024-byte pass on both sides."""
    if n == 1:
        return [(1025, 1031)]
    m = len(MATE_LENGTHS)
    lens = [(MATE_LENGTHS[(i + 3) % m], MATE_LENGTHS[(i // m * 5 + i * 7) % m]) for i in range(n)]
    lens[:len(MATES_SPECIAL)] = MATES_SPECIAL
    return lens


_CACHE = {}


def mates_batch(n, lead, base):
    key = ("mates", n, lead, base)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * n + 10 * lead + base)
        reads = [random_read(rng, length) for pair in mates_lengths(n) for length in pair]
        _CACHE[key] = make_batch(reads, lead, base, seed=n, name=f"{n} pairs, lead {lead}, base {base}")
    return _CACHE[key]


def mates_bad_batch():
    """65 pairs with two whose offsets are out of order between good ones: pair 7 has m < b, pair 41 has e < m."""
    if "bad" not in _CACHE:
        good = mates_batch(65, 1, 3)
        offsets = good.offsets.copy()
        offsets[2 * 7 + 1] = offsets[2 * 7] - np.uint64(1)
        offsets[2 * 41 + 1] = offsets[2 * 41 + 2] + np.uint64(5)
        _CACHE["bad"] = (Batch(good.buffer, good.lead, offsets, good.reads, "65 pairs, two with offsets out of order"), (7, 41))
    return _CACHE["bad"]


def _latin(b):
    return b.decode("latin-1")


def joined_sequences(batch, orientation, sep, bad=()):
    """Per pair (J as bytes, which bytes of it are closed).  J of a pair the kernel must leave alone: FILL over its range."""
    out = []
    for i in range(len(batch.reads) // 2):
        m1, m2 = batch.reads[2 * i], batch.reads[2 * i + 1]
        if i in bad:
            size = int(batch.offsets[2 * i + 2] - batch.offsets[2 * i]) + 1
            out.append((bytes([FILL]) * size, np.ones(size, dtype=bool)))
            continue
        j = mates.join(_latin(m1), _latin(m2), orientation, chr(sep)).encode("latin-1")
        closed = np.ones(len(j), dtype=bool)
        if orientation == "fr":
            closed[len(m1) + 1:] = False        # rc(m2): defined by class
        out.append((j, closed))
    return out


def joined_pattern(batch, orientation, sep, bad=()):
    """J_0 J_1 ... dense, as the joined offsets seq_offsets[2 i] - seq_offsets[0] + i put them."""
    seqs = joined_sequences(batch, orientation, sep, bad)
    segments, at = [], 0
    for i, (j, _) in enumerate(seqs):
        l1, l2 = len(batch.reads[2 * i]), len(batch.reads[2 * i + 1])
        how = "copied" if orientation == "ff" else "reversed, by class"
        segments += [(at, f"{batch.name}: pair {i}, mate 1 ({l1} bytes)"), (at + l1, f"{batch.name}: pair {i}, the separator"),
                     (at + l1 + 1, f"{batch.name}: pair {i}, mate 2 ({l2} bytes, {how})")]
        if i in bad:
            segments[-3:] = [(at, f"{batch.name}: pair {i}, whose offsets are out of order (left as it was)")]
        at += len(j)
    exact = np.frombuffer(b"".join(j for j, _ in seqs), dtype=np.uint8)
    return Pattern(exact, np.concatenate([c for _, c in seqs]), segments)


def joined_offsets(batch):
    n = len(batch.reads) // 2
    return [int(batch.offsets[2 * i]) - batch.base + i for i in range(n)] + [int(batch.offsets[2 * n]) - batch.base + n]


def reversed_pattern(seqs, names, lead_fill=0):
    """rc(s_0) rc(s_1) ... dense, every byte by class; lead_fill bytes of FILL in front (what lies below seq_offsets[0])."""
    parts = [bytes([FILL]) * lead_fill] + [rc(s) for s in seqs]
    segments, at = [(0, "the bytes below seq_offsets[0]")] if lead_fill else [], lead_fill
    for s, name in zip(seqs, names):
        segments.append((at, f"{name} reversed ({len(s)} bytes, by class)"))
        at += len(s)
    closed = np.zeros(at, dtype=bool)
    closed[:lead_fill] = True
    return Pattern(np.frombuffer(b"".join(parts), dtype=np.uint8), closed, segments)


def copy_alignments(batch, orientation):
    """(source & 3, destination & 3) of every copy_forward of a whole dword and more: mate 1's, and mate 2's in FF.  The
    allocation and the joined region are 256-byte aligned, so the low bits are those of the offsets."""
    seen = {1: set(), 2: set()}
    for i, at in enumerate(joined_offsets(batch)[:-1]):
        l1, l2 = len(batch.reads[2 * i]), len(batch.reads[2 * i + 1])
        copies = [(1, batch.address(2 * i), at, l1)] + ([(2, batch.address(2 * i + 1), at + l1 + 1, l2)] if orientation == "ff" else [])
        for mate, src, dst, length in copies:
            head = min(length, (4 - (dst & 3)) & 3)
            if (length - head) // 4 >= 1:
                seen[mate].add((src & 3, dst & 3))
    return seen


# ---- strands ------------------------------------------------------------------------------------------------------------
STRAND_CASES = ((1, 0, 0), (63, 1, 0), (64, 0, 0), (65, 2, 0), (257, 3, 0), (65, 1, 4099))


def strand_batch(n, lead, base):
    key = ("strand", n, lead, base)
    if key not in _CACHE:
        rng = np.random.default_rng(2000 * n + 10 * lead + base)
        lengths = [1025] if n == 1 else [STRAND_LENGTHS[(i * 5 + 1) % len(STRAND_LENGTHS)] for i in range(n)]
        _CACHE[key] = make_batch([random_read(rng, length, rich=0.25) for length in lengths], lead, base, seed=n,
                                 name=f"{n} reads, lead {lead}, base {base}")
    return _CACHE[key]


# ---- frames -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _memoized_codons():
    """test_translate_cpu's translation with its two pure per-character and per-codon functions memoized while it runs (they
    are looked up at each call): the same strings, ten times sooner on reads of 2 306 nucleotides."""
    saved = test_translate_cpu.nucl_class, test_translate_cpu.residue_of_classes
    test_translate_cpu.nucl_class = functools.lru_cache(maxsize=None)(saved[0])
    test_translate_cpu.residue_of_classes = functools.lru_cache(maxsize=None)(saved[1])
    try:
        yield
    finally:
        test_translate_cpu.nucl_class, test_translate_cpu.residue_of_classes = saved


_FRAMES = {}


def cached_frames(read, mode):
    """test_translate_cpu.frames(read, mode), computed once a read (all six; a mode's frames are a slice of them)."""
    if read not in _FRAMES:
        with _memoized_codons():
            _FRAMES[read] = tuple(frames(read, "both"))
    return list(_FRAMES[read][{"forward": slice(0, 3), "reverse": slice(3, 6), "both": slice(0, 6)}[mode]])


def long_read(rng, length, index):
    """A read over one, two or three windows, with a motif of MOTIFS on the codons over either seam (moved by 0, 1 or 2)."""
    read = bytearray(random_read(rng, length, rich=0.05))
    for w, first in enumerate((764, 1532)):
        motif = MOTIFS[(index + 4 * w) % len(MOTIFS)]
        at = first + (index // len(MOTIFS)) % 3
        if at + len(motif) <= length:
            read[at:at + len(motif)] = motif
        elif at < length:                       # (L = 769 .. 771: the read ends inside the motif)
            read[at:] = motif[:length - at]
    return bytes(read)


SHORT_READS = (b"", b"A", b"AC", b"ACG", b"TAAG", b"RAYSA", b"SARMTH", b"MTHTAAu", b"a-GNNNTG")     # L = 0 .. 8


def frame_pool():
    """Every long length at each of the 16 values of (address of the read's first byte) & 15, set by a filler read of 0 .. 15
    bytes in front of it; then L = 0 .. 8.  (The batch of the whole pool starts at address 0.)"""
    if "pool" not in _CACHE:
        rng = np.random.default_rng(31)
        reads, at = [], 0
        for li, length in enumerate(FRAME_LONG):
            for a in range(16):
                filler = random_read(rng, (a - at) % 16, rich=0.3)
                reads += [filler, long_read(rng, length, 16 * li + a)]
                at += len(filler) + length
        _CACHE["pool"] = reads + list(SHORT_READS)
    return _CACHE["pool"]


# name: (slice of the pool, lead, base)
FRAME_CASES = {"pool": (slice(None), 0, 0), "one": (slice(259, 260), 5, 0), "n63": (slice(10, 73), 1, 0), "n64": (slice(100, 164), 7, 0),
               "n65": (slice(200, 265), 11, 0), "n257": (slice(40, 297), 2, 0), "base": (slice(150, 215), 3, 4099)}


def frame_batch(name):
    key = ("frames", name)
    if key not in _CACHE:
        part, lead, base = FRAME_CASES[name]
        _CACHE[key] = make_batch(frame_pool()[part], lead, base, seed=len(name), name=f"frames '{name}'")
    return _CACHE[key]


def frames_pattern(batch, mode):
    """The frames of read 0, then of read 1, ...: synth.pack_reads([f for r in reads for f in frames(r, mode)]), every byte."""
    names = test_translate_cpu.FRAME_NAMES[3:] if mode == "reverse" else test_translate_cpu.FRAME_NAMES
    parts, segments, offsets, at = [], [], [0], 0
    for i, read in enumerate(batch.reads):
        for name, f in zip(names, cached_frames(_latin(read), mode)):
            segments.append((at, f"{batch.name}: read {i} (L = {len(read)}, address & 15 = {batch.address(i) & 15}), frame {name}"))
            parts.append(f.encode("latin-1"))
            at += len(f)
            offsets.append(at)
    return Pattern(np.frombuffer(b"".join(parts), dtype=np.uint8), None, segments), offsets


# ---- the selection kernels ----------------------------------------------------------------------------------------------
def selection_reads(kind):
    """257 reads (strands, frames) or pairs (mates, interleaved: 514 reads) of ordinary length, some too short to have rows."""
    key = ("selection", kind)
    if key not in _CACHE:
        rng = np.random.default_rng({"strands": 51, "mates": 52, "frames": 53}[kind])
        if kind == "frames":
            lengths = [int(rng.integers(0, 8)) if i % 9 == 4 else int(rng.integers(12, 90)) for i in range(257)]
        elif kind == "strands":
            lengths = [int(rng.integers(0, 4)) if i % 9 == 4 else int(rng.integers(4, 80)) for i in range(257)]
        else:   # (a pair without rows: J shorter than k = 4)
            lengths = [int(rng.integers(0, 2)) if i % 18 in (8, 9) else int(rng.integers(0, 60)) for i in range(514)]
        _CACHE[key] = ["".join(rng.choice(list("ACGT"), size=m)) for m in lengths]
    return _CACHE[key]


def selection_kinds(label, n_rows):
    """Per read: 'later' (the reverse strand or a frame behind the mode's first wins), 'first', or 'none' (no rows)."""
    rows = (n_rows != 0) & (n_rows != capi.ROWS_COUNTS_TOO_NARROW)
    return np.where(~rows, "none", np.where(label != 0, "later", "first"))


def selection_singles(kinds):
    """The batches of ONE read: the first read of each kind."""
    return [int(np.nonzero(kinds == kind)[0][0]) for kind in ("later", "first", "none")]


def nucl_db():
    if "nucl_db" not in _CACHE:
        _CACHE["nucl_db"] = synth.make_db(synth.make_tree(40, seed=21).num_nodes, kmer_size=4, p_present=0.7, seed=22,
                                          lognormal=(1.0, 1.0))      # 79 branches
    return _CACHE["nucl_db"]


def amino_db():
    if "amino_db" not in _CACHE:
        _CACHE["amino_db"] = synth.make_db(synth.make_tree(30, seed=8).num_nodes, states="amino", kmer_size=3, seed=12,
                                           p_present=0.4, lognormal=(1.5, 1.0))   # 59 branches
    return _CACHE["amino_db"]


def selection_reference(oracle_lib, kind, keep, factor):
    """(rows, n_rows, counts), label of the whole pool under the `both` rule, from the oracle; computed once and read-only."""
    from test_strand_gpu import both_rule            # (the rule on two oracle runs; the module needs no GPU to import)
    from test_translate_gpu import oracle_frames
    key = ("selection ref", kind, keep, factor)
    if key not in _CACHE:
        reads = selection_reads(kind)
        if kind == "frames":
            orc = oracle_lib.Oracle.from_synth(amino_db(), keep_at_most=keep, keep_factor=factor)
            want, label = oracle_frames(orc, reads, "both", amino_db().kmer_size, keep)
        else:
            orc = oracle_lib.Oracle.from_synth(nucl_db(), keep_at_most=keep, keep_factor=factor)
            seqs = reads if kind == "strands" else [mates.join(a, b) for a, b in zip(reads[0::2], reads[1::2])]
            fwd = orc.place(*synth.pack_reads(seqs), num_threads=0)
            rev = orc.place(*synth.pack_reads([mates.reverse_complement(s) for s in seqs]), num_threads=0)
            want, label = both_rule(fwd, rev)
        for a in want + (label,):
            a.setflags(write=False)
        _CACHE[key] = (want, label)
    return _CACHE[key]


# ---- (1) the mates reach every alignment, length and seam -----------------------------------------------------------
def test_mate_lengths_cover_both_sides_and_the_empty_mates():
    for n in BATCH_SIZES[1:]:
        lens = mates_lengths(n)
        assert len(lens) == n and {a for a, _ in lens} == set(MATE_LENGTHS) == {b for _, b in lens}
        assert (0, 0) in lens and any(a == 0 < b for a, b in lens) and any(b == 0 < a for a, b in lens)
    assert {n for n, _, _ in MATES_CASES} == set(BATCH_SIZES)
    assert {(lead, base) for _, lead, base in MATES_CASES} >= {(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3)}
    assert max(base for _, _, base in MATES_CASES) > 4096
    # a pass of copy_forward is 1 024 bytes, of the reversal 256: lengths on both sides of one and of four passes
    assert {255, 256, 257, 1023, 1024, 1025} <= set(MATE_LENGTHS)


@pytest.mark.parametrize("orientation", ["fr", "ff"])
def test_every_pair_of_source_and_destination_alignment_occurs(orientation):
    every = {(s, d) for s in range(4) for d in range(4)}
    seen = {1: set(), 2: set()}
    for case in MATES_CASES:
        got = copy_alignments(mates_batch(*case), orientation)
        seen = {m: seen[m] | got[m] for m in seen}
        if case[0] >= 63:        # (one batch alone reaches them all: the pair index moves the destination against the source)
            assert got[1] == every and (orientation == "fr" or got[2] == every), case
    assert seen[1] == every
    assert seen[2] == (every if orientation == "ff" else set())


def test_joined_bytes_are_the_rule_and_open_only_where_the_complement_is():
    batch, sep = mates_batch(63, 1, 0), ord("-")
    for orientation in ("fr", "ff"):
        pattern = joined_pattern(batch, orientation, sep)
        at = 0
        for i, (j, closed) in enumerate(joined_sequences(batch, orientation, sep)):
            m1, m2 = batch.reads[2 * i], batch.reads[2 * i + 1]
            assert j[:len(m1) + 1] == m1 + b"-" and closed[:len(m1) + 1].all() and len(j) == len(m1) + len(m2) + 1
            second = np.frombuffer(j[len(m1) + 1:], dtype=np.uint8)
            if orientation == "ff":
                assert second.tobytes() == m2 and closed.all()
            else:   # the class at position t is the bit-reversed class of mate 2's byte len - 1 - t (include/epik_amd.h)
                assert np.array_equal(NUCL_CLASS[second], BITREV[NUCL_CLASS[np.frombuffer(m2, dtype=np.uint8)[::-1]]])
                assert not closed[len(m1) + 1:].any()
            assert pattern.exact[at:at + len(j)].tobytes() == j and joined_offsets(batch)[i] == at
            at += len(j)
        assert joined_offsets(batch)[-1] == at == pattern.exact.size
        assert FILL not in pattern.exact
    bad_batch, bad = mates_bad_batch()
    o = bad_batch.offsets.astype(np.int64)
    assert o[15] < o[14] and o[84] < o[83] and all(o[2 * i] <= o[2 * i + 1] <= o[2 * i + 2] for i in range(65) if i not in bad)
    pattern = joined_pattern(bad_batch, "fr", sep, bad)
    assert joined_offsets(bad_batch) == joined_offsets(mates_batch(65, 1, 3))
    for i in bad:
        a, b = joined_offsets(bad_batch)[i:i + 2]
        assert b - a > 64 and (pattern.exact[a:b] == FILL).all() and pattern.closed[a:b].all()
    assert int((pattern.exact == FILL).sum()) == sum(joined_offsets(bad_batch)[i + 1] - joined_offsets(bad_batch)[i] for i in bad)


# ---- (2) the strands ------------------------------------------------------------------------------------------------
def test_strand_batches_hold_every_length_and_alphabet():
    assert {n for n, _, _ in STRAND_CASES} == set(BATCH_SIZES) and any(base for _, _, base in STRAND_CASES)
    for case in STRAND_CASES[1:]:
        batch = strand_batch(*case)
        assert {len(r) for r in batch.reads} == set(STRAND_LENGTHS)
        text = b"".join(batch.reads)
        assert set(RICH) <= set(text) and FILL not in text
        pattern = reversed_pattern(batch.reads, [f"read {i}" for i in range(case[0])], lead_fill=min(batch.base, 64))
        fill = min(batch.base, 64)
        assert (pattern.exact[:fill] == FILL).all() and pattern.closed[:fill].all() and not pattern.closed[fill:].any()
        assert pattern.exact.size == fill + len(text)
        for i, read in enumerate(batch.reads):     # the class at position t: the bit-reversed class of the read's byte len - 1 - t
            a = fill + int(batch.offsets[i]) - batch.base
            got = NUCL_CLASS[pattern.exact[a:a + len(read)]]
            assert np.array_equal(got, BITREV[NUCL_CLASS[np.frombuffer(read, dtype=np.uint8)[::-1]]])
    assert len(strand_batch(1, 0, 0).reads[0]) == 1025 and (strand_batch(65, 1, 4099).base, strand_batch(65, 1, 4099).lead) == (4099, 1)


# ---- (3) the frames -------------------------------------------------------------------------------------------------
def test_every_load_shift_and_length_residue_occurs_at_every_window_seam():
    assert K_TILE % 16 == 0        # a read's windows all load with the shift of its first byte
    batch = frame_batch("pool")
    seen = {seam: set() for seam in FRAME_SEAMS}
    for i, read in enumerate(batch.reads):
        for seam, lengths in FRAME_SEAMS.items():
            if len(read) in lengths:
                seen[seam].add((batch.address(i) & 15, len(read) % 3))
    for seam, lengths in FRAME_SEAMS.items():
        assert seen[seam] == {(s, r) for s in range(16) for r in range(3)}, seam
        # T = L - 2 codon starts: one below, at, and above `seam` whole windows
        assert {L - 2 - seam * K_TILE for L in lengths} >= {-1, 0, 1}
    for length in FRAME_LONG:      # every long length at each of the 16 alignments of its first byte
        assert {batch.address(i) & 15 for i, r in enumerate(batch.reads) if len(r) == length} == set(range(16)), length
    assert {len(r) for r in batch.reads} >= set(range(9)) | set(FRAME_LONG)
    assert {len(frame_batch(name).reads) for name in FRAME_CASES} >= set(BATCH_SIZES)
    assert len(frame_batch("one").reads[0]) == 2306 and frame_batch("base").base > 4096
    for name in FRAME_CASES:       # every batch has reads over a seam
        assert max(len(r) for r in frame_batch(name).reads) > K_TILE + 2, name


def test_the_codons_over_the_seams_carry_information_in_both_directions():
    long_reads = [r for r in frame_pool() if len(r) > K_TILE]
    assert len(long_reads) == 16 * len(FRAME_LONG)
    stops, reverse_stops = (b"TAA", b"TAG", b"TGA"), (b"TTA", b"CTA", b"TCA")
    for positions in SEAM_POSITIONS:
        at = [bytes(r[p] for p in positions if p < len(r)) for r in long_reads if len(r) > positions[0]]
        text = b"".join(at)
        classes = NUCL_CLASS[np.frombuffer(text, dtype=np.uint8)]
        assert (classes == 0).any() and (np.bincount(classes, minlength=16)[[3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]] > 0).sum() >= 6
        assert any(c in text for c in b"acgt") and any(c in text for c in b"Uu")
        # a stop on a codon that starts at most two nucleotides before the first lookahead byte, forward and reverse
        first = positions[2]            # 768 | 1 536: the first codon start of the next window
        for codons in (stops, reverse_stops):
            assert any(r[j:j + 3] in codons for r in long_reads for j in range(first - 2, first + 1) if j + 3 <= len(r))
    # ... and so do the expected frames: the residues of the codons over the first seam
    near = set()
    for read in long_reads:
        near |= set("".join(f[(764 - 2) // 3:775 // 3 + 1] for f in cached_frames(_latin(read), "forward")))
    assert near >= set("BZJX*"), near


def test_expected_frames_hold_every_residue_letter_and_are_the_translation():
    batch = frame_batch("pool")
    for mode in ("forward", "reverse", "both"):
        pattern, offsets = frames_pattern(batch, mode)
        assert {chr(c) for c in set(pattern.exact.tolist())} == RESIDUES, mode
        m = 6 if mode == "both" else 3
        assert len(offsets) == m * len(batch.reads) + 1 and offsets[-1] == pattern.exact.size
        assert pattern.exact.size == (m // 3) * sum(max(len(r) - 2, 0) for r in batch.reads)
    # the memoized translation is test_translate_cpu's own
    for read in (frame_pool()[1], frame_pool()[-1], frame_pool()[-3]):
        assert cached_frames(_latin(read), "both") == frames(_latin(read), "both")
        assert cached_frames(_latin(read), "reverse") == frames(_latin(read), "reverse")
    data, offs = synth.pack_reads([f for r in frame_batch("n63").reads for f in cached_frames(_latin(r), "both")])
    pattern, offsets = frames_pattern(frame_batch("n63"), "both")
    assert data.tobytes() == pattern.exact.tobytes() and offs.tolist() == offsets


# ---- (4) the selection batches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["strands", "mates", "frames"])
def test_selection_batches_hold_both_winners_and_reads_without_rows(oracle_lib, kind):
    for keep, factor in EDGE_KEEPS:
        (rows, n_rows, counts), label = selection_reference(oracle_lib, kind, keep, factor)
        assert rows.shape == (257, keep)
        kinds = selection_kinds(label, n_rows)
        for n in BATCH_SIZES[1:]:
            found = {k: int((kinds[:n] == k).sum()) for k in ("later", "first", "none")}
            assert min(found.values()) >= 3, (kind, keep, n, found)
        singles = selection_singles(kinds)
        assert [kinds[i] for i in singles] == ["later", "first", "none"]
        assert int(n_rows.max()) == keep if keep == 1 else 1 < int(n_rows.max()) <= keep
        if kind == "frames":      # every frame wins somewhere
            assert set(label[kinds != "none"].tolist()) == set(range(6))


# ---- (5) a wrong byte is found and named -----------------------------------------------------------------------------
def test_locate_names_the_first_wrong_byte():
    batch, sep = mates_batch(64, 2, 0), ord("-")
    pattern = joined_pattern(batch, "fr", sep)
    ws = np.full(pattern.exact.size + 3000, FILL, dtype=np.uint8)
    # what the library writes: the smallest byte of the complemented class where the class decides
    smallest = np.array([int(np.nonzero(NUCL_CLASS == c)[0][0]) for c in range(16)], dtype=np.uint8)
    written = np.where(pattern.closed, pattern.exact, smallest[NUCL_CLASS[pattern.exact]])
    assert (written != pattern.exact).any()
    ws[1024:1024 + written.size] = written
    assert locate(ws, pattern, "joined") == (1024, None)
    pair = 24
    start = joined_offsets(batch)[pair]
    l1 = len(batch.reads[2 * pair])
    assert l1 >= 8
    for where, offset, text in (("mate 1", 5, f"pair {pair}, mate 1 ({l1} bytes), position 5 of it"),
                                ("mate 2", l1 + 1 + 2, f"pair {pair}, mate 2 ({len(batch.reads[2 * pair + 1])} bytes, reversed, by class), position 2")):
        wrong = ws.copy()
        at = 1024 + start + offset
        wrong[at] = ord("A") if VIEW[wrong[at]] != VIEW[ord("A")] else ord("C")
        position, message = locate(wrong, pattern, "joined")
        assert position == -1 and text in message, message
    # the very first byte wrong: no prefix occurs, the string is laid where its suffix puts it
    wrong = ws.copy()
    wrong[1024] = ord("A")
    position, message = locate(wrong, pattern, "joined")
    assert position == -1 and "laid over byte 1024 of it, 1 of" in message and "pair 0, the separator, position 0 of it" in message, message
    # the same class in another case: wrong where the byte counts, right where the class does
    lower = ws.copy()
    at = 1024 + start + int(np.nonzero(np.isin(pattern.exact[start:start + l1], list(b"ACGT")))[0][0])
    lower[at] = lower[at] + 32
    position, message = locate(lower, pattern, "joined")
    assert position == -1 and "the classes are found at byte 1024" in message and f"pair {pair}, mate 1" in message, message
    # a pair left out leaves FILL behind: found by its first byte
    short = ws.copy()
    short[1024 + start:1024 + joined_offsets(batch)[pair + 1]] = FILL
    position, message = locate(short, pattern, "joined")
    assert position == -1 and f"pair {pair}, mate 1 ({l1} bytes), position 0 of it" in message and ": 0xa5, expected" in message, message
    offsets = offsets_pattern(joined_offsets(batch), "joined_offsets")
    table = np.concatenate([np.full(64, FILL, dtype=np.uint8), offsets.exact])
    assert locate(table, offsets, "offsets") == (64, None)
    table[64 + 8 * 9] ^= 1
    assert "joined_offsets[9]" in locate(table, offsets, "offsets")[1]
