"""Host-side mirror of `epik::placer` (reference epik/include/epik/place.h:81-140)
over the C-ABI of libepik_amd.so.

Same constructor arguments and `place()` contract as the reference class:

    placer(db, tree, keep_at_most, keep_factor, max_threads)      place.h:94-95
    placed_collection place(seq_records, num_threads)              place.h:103

* the constructor precomputes the pendant lengths (place.cpp:99-125) and uploads
  the database to HBM through `epik_amd_placer_create`;
* `place()` groups identical sequences (place.cpp:73-81, 207-212), sends the unique
  reads through the boundary, and joins distal/pendant lengths onto the returned
  rows (place.cpp:435-437).

The heavy lifting is the HIP kernel; nothing here computes a score.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Iterable, List, Sequence, Tuple

import numpy as np

from . import alphabet, capi
from .mates import check_mate_names


@dataclass
class Placement:
    """`epik::impl::placement` (place.h:45-56)."""

    branch_id: int
    score: float          # float32 value
    weight_ratio: float   # double
    count: int
    distal_length: float
    pendant_length: float


@dataclass
class PlacedSequence:
    """`epik::impl::placed_sequence` (place.h:59-68)."""

    sequence: str
    placements: List[Placement]
    strand: str = "+"     # the strand placed: "-" when the reverse complement won (Placer.place(strand=...))
    frame: str = ""       # the frame placed, "+1" ... "-3" (Placer.place(translate=...)); "" when not translated
    mate: str = None      # mate 2 as given, when a pair was placed (Placer.place(mates=...)): `sequence` is mate 1


@dataclass
class PlacedCollection:
    """`epik::impl::placed_collection` (place.h:72-75): sequence -> headers, plus
    one PlacedSequence per unique sequence (first-occurrence order; the reference's
    order is std::unordered_map iteration order, place.cpp:57-61)."""

    sequence_map: dict
    placed_seqs: List[PlacedSequence]
    #: Placer.place(assign=...): the confidence record of every placed sequence (capi.CONFIDENCE), in their order
    confidence: np.ndarray = field(default=None, compare=False)


def pendant_lengths(branch_length: np.ndarray, subtree_num_nodes: np.ndarray,
                    subtree_total_length: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(distal, pendant) per post-order id, place.cpp:99-125 / :435."""
    branch_length = np.asarray(branch_length, dtype=np.float64)
    num = np.asarray(subtree_num_nodes, dtype=np.float64)
    tot = np.asarray(subtree_total_length, dtype=np.float64)
    distal = branch_length / 2                      # :110
    mean = np.where(num > 1, tot / np.maximum(num, 1), 0.0)  # :117-121
    return distal, mean + distal                    # :123


def make_desc(offsets, values, *, states: str, kmer_size: int, num_branches: int, threshold, log_threshold=None,
              keep_at_most: int = 7, keep_factor: float = 0.01, device: int = 0, char_class=None, keys=None,
              sparse: bool = False, holds_shard=None):
    """`epik_amd_placer_desc` over host arrays (uint32 / uint64 offsets are handed over as they are, no
    copy).  `keys` (ascending uint32 codes that have a list): the sparse form, `offsets` then has
    len(keys) + 1 entries; `sparse=True` turns dense offsets into that form first (EPIK_AMD_SPARSE_DESC=1
    does it for every descriptor: the GPU tests run on both forms).  `holds_shard=(g, G)`: the arrays hold shard g of
    G of a database already (only the lists of the codes with code % G == g: `epik_amd_placer_desc.shard`).
    Returns (desc, the arrays it points into -- keep them alive as long as the descriptor)."""
    sigma = alphabet.alphabet_size(states)
    if log_threshold is None:
        log_threshold = alphabet.log_threshold(np.float32(threshold))
    offsets = np.asarray(offsets)
    num_keys = sigma ** int(kmer_size)
    if keys is None and (sparse or os.environ.get("EPIK_AMD_SPARSE_DESC") == "1"):
        lens = np.diff(offsets.astype(np.int64))
        present = np.nonzero(lens)[0]
        keys = present.astype(np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lens[present])]).astype(np.uint64)
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        assert offsets.shape[0] == keys.shape[0] + 1
    num_entries = int(offsets[-1])
    if offsets.dtype == np.uint64 and offsets.flags.c_contiguous:
        off, bits = offsets, 64
    elif num_entries <= 0xFFFFFFFF:
        off, bits = np.ascontiguousarray(offsets, dtype=np.uint32), 32
    else:
        off, bits = np.ascontiguousarray(offsets, dtype=np.uint64), 64
    vals = np.ascontiguousarray(values)
    if vals.dtype.itemsize != 8:
        raise ValueError("values must be 8-byte {uint32 branch, float32 score} records")
    cls = np.ascontiguousarray(
        alphabet.char_class_table(states) if char_class is None else char_class, dtype=np.uint32)
    desc = capi.PlacerDesc(
        abi_version=capi.ABI_VERSION, kmer_size=int(kmer_size), alphabet_size=sigma,
        num_branches=int(num_branches), keep_at_most=int(keep_at_most), offset_bits=bits,
        keep_factor=float(keep_factor), threshold=float(threshold),
        log_threshold=float(log_threshold), num_keys=int(num_keys),
        num_entries=num_entries, offsets=off.ctypes.data, values=vals.ctypes.data,
        char_class=cls.ctypes.data, device=int(device),
        shard=0 if holds_shard is None or int(holds_shard[1]) <= 1 else (int(holds_shard[0]) | int(holds_shard[1]) << 16),
        keys=keys.ctypes.data if keys is not None else None, num_present=int(keys.shape[0]) if keys is not None else 0)
    return desc, (off, vals, cls, keys)


def plan(db, *, shard_index: int = 0, shard_count: int = 1, free_bytes: int = 288 << 30, **kw) -> capi.Plan:
    """`epik_amd_placer_plan`: kernel, layout and device-image sizes create() would choose for a
    synthetic / loaded database `db` -- no device needed."""
    kw.setdefault("keys", getattr(db, "keys", None))
    kw.setdefault("holds_shard", getattr(db, "shard", None))
    desc, keep = make_desc(db.offsets, db.values, states=db.states, kmer_size=db.kmer_size,
                           num_branches=db.num_branches, threshold=db.threshold, log_threshold=db.log_threshold, **kw)
    out = capi.Plan()
    capi.check(capi.load().epik_amd_placer_plan(ctypes.byref(desc), shard_index, shard_count, int(free_bytes),
                                                ctypes.byref(out)))
    del keep
    return out


def plan_sizes(*, states: str, kmer_size: int, num_branches: int, bins, keep_at_most: int = 7, shard_index: int = 0,
               shard_count: int = 1, free_bytes: int = 288 << 30) -> capi.Plan:
    """`epik_amd_placer_plan_sizes`: the plan of a database known by its SIZES only -- `bins` = (length, lists[,
    lists_in_runs]) per length of posting list the placer (its shard) keeps.  No device, no postings."""
    arr = (capi.ListBin * max(len(bins), 1))()
    for i, b in enumerate(bins):
        arr[i].length, arr[i].lists = int(b[0]), int(b[1])
        arr[i].lists_in_runs = int(b[2]) if len(b) > 2 else 0
    out = capi.Plan()
    capi.check(capi.load().epik_amd_placer_plan_sizes(int(kmer_size), alphabet.alphabet_size(states), int(num_branches),
                                                      int(keep_at_most), arr, len(bins), int(shard_index), int(shard_count),
                                                      int(free_bytes), ctypes.byref(out)))
    return out


def list_bins(db, shard_index: int = 0, shard_count: int = 1):
    """The histogram `plan_sizes` takes, of a database at hand (tests; capacity reports of a loaded database)."""
    offsets = np.asarray(db.offsets).astype(np.int64)
    lens = np.diff(offsets)
    codes = np.asarray(db.keys, dtype=np.int64) if getattr(db, "keys", None) is not None else np.arange(len(lens))
    mine = (codes % shard_count == shard_index) & (lens > 0)
    br = db.values["branch"].astype(np.int64)
    steps_ok = np.ones(len(br), dtype=bool)
    steps_ok[1:] = np.diff(br) == 1
    broken = np.zeros(len(br) + 1, dtype=np.int64)   # (how many positions of a list other than its first break the run)
    inner = np.ones(len(br), dtype=bool)
    inner[offsets[:-1][lens > 0]] = False
    broken[1:] = np.cumsum(~steps_ok & inner)
    is_run = (broken[offsets[1:]] - broken[offsets[:-1]] == 0) & (lens > 0) & (lens < 65536)
    out = []
    for length in np.unique(lens[mine]):
        sel = mine & (lens == length)
        out.append((int(length), int(sel.sum()), int((sel & is_run).sum())))
    return out


def build_image(db, *, shard_index: int = 0, shard_count: int = 1, free_bytes: int = 288 << 30, discard=False, **kw):
    """`epik_amd_placer_build_image`: the device image as three uint8 arrays (table, filter, postings);
    with `discard` the image is produced and dropped (returns the plan only).  Host only."""
    kw.setdefault("keys", getattr(db, "keys", None))
    kw.setdefault("holds_shard", getattr(db, "shard", None))
    desc, keep = make_desc(db.offsets, db.values, states=db.states, kmer_size=db.kmer_size,
                           num_branches=db.num_branches, threshold=db.threshold, log_threshold=db.log_threshold, **kw)
    lib = capi.load()
    p = capi.Plan()
    capi.check(lib.epik_amd_placer_plan(ctypes.byref(desc), shard_index, shard_count, int(free_bytes), ctypes.byref(p)))
    parts = [None, None, None] if discard else [np.zeros(int(n), dtype=np.uint8)
                                                for n in (p.table_bytes, p.filter_bytes, p.posting_bytes)]
    ptr = [None if a is None or a.size == 0 else a.ctypes.data for a in parts]
    capi.check(lib.epik_amd_placer_build_image(ctypes.byref(desc), shard_index, shard_count, int(free_bytes), *ptr))
    del keep
    return (p, *parts)


class Placer:
    """MI355X placer.  `offsets`/`values` are the CSR database (host arrays),
    `branch_length`/`subtree_*` the per-post-order-id tree data (may be None when
    only raw rows are wanted)."""

    def __init__(self, offsets: np.ndarray, values: np.ndarray, *, states: str, kmer_size: int,
                 num_branches: int, threshold, log_threshold=None, keep_at_most: int = 7,
                 keep_factor: float = 0.01, device: int = 0, branch_length=None,
                 subtree_num_nodes=None, subtree_total_length=None, char_class=None,
                 shard_index: int = 0, shard_count: int = 1, keys=None, sparse: bool = False, holds_shard=None):
        lib = capi.load()
        sigma = alphabet.alphabet_size(states)
        self.states = states
        self.kmer_size = int(kmer_size)
        self.num_branches = int(num_branches)
        self.keep_at_most = int(keep_at_most)
        self.keep_factor = float(keep_factor)
        self.device = int(device)
        desc, keepalive = make_desc(
            offsets, values, states=states, kmer_size=kmer_size, num_branches=num_branches, threshold=threshold,
            log_threshold=log_threshold, keep_at_most=keep_at_most, keep_factor=keep_factor, device=device,
            char_class=char_class, keys=keys, sparse=sparse, holds_shard=holds_shard)
        handle = ctypes.c_void_p()
        # shard_count > 1: this placer keeps the posting lists of the codes with
        # code % shard_count == shard_index (k-mer-space shard, `epik_amd_placer_create_sharded`)
        self.shard_index, self.shard_count = int(shard_index), int(shard_count)
        capi.check(lib.epik_amd_placer_create_sharded(ctypes.byref(desc), self.shard_index, self.shard_count,
                                                      ctypes.byref(handle)))
        del keepalive  # create() has streamed the database to the device and keeps no host copy
        self._lib = lib
        self._handle = handle
        if branch_length is not None:
            if len(branch_length) != self.num_branches:
                # place.cpp:104-108: "Could not find node by post-order id"
                raise RuntimeError(
                    f"Could not find node by post-order id: {min(len(branch_length), self.num_branches)}")
            self.distal, self.pendant = pendant_lengths(branch_length, subtree_num_nodes,
                                                        subtree_total_length)
        else:
            self.distal = self.pendant = None

    @classmethod
    def from_synth(cls, db, tree=None, **kw):
        extra = {}
        if tree is not None:
            extra = dict(branch_length=tree.branch_length, subtree_num_nodes=tree.subtree_num_nodes,
                         subtree_total_length=tree.subtree_total_length)
        kw.setdefault("keys", getattr(db, "keys", None))
        kw.setdefault("holds_shard", getattr(db, "shard", None))   # (synth.make_db(shard=...): one shard's lists only)
        return cls(db.offsets, db.values, states=db.states, kmer_size=db.kmer_size,
                   num_branches=db.num_branches, threshold=db.threshold,
                   log_threshold=db.log_threshold, **extra, **kw)

    # -- lifetime -----------------------------------------------------------------
    def close(self):
        if getattr(self, "_handle", None):
            self._lib.epik_amd_placer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the boundary, raw ----------------------------------------------------------
    def place_packed(self, seqs: np.ndarray, seq_offsets: np.ndarray):
        """Host buffers in, host buffers out (`epik_amd_placer_place`).  Returns
        (rows[n, keep] PLACEMENT, n_rows[n] uint32, kmer_counts[n, keep] uint32)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        rows = np.zeros((n, self.keep_at_most), dtype=capi.PLACEMENT)
        n_rows = np.zeros(n, dtype=np.uint32)
        counts = np.zeros((n, self.keep_at_most), dtype=np.uint32)
        capi.check(self._lib.epik_amd_placer_place(
            self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, rows.ctypes.data,
            n_rows.ctypes.data, counts.ctypes.data))
        return rows, n_rows, counts

    def place_device(self, d_seqs: int, d_seq_offsets: int, n: int, d_rows: int, d_n_rows: int,
                     d_kmer_counts: int = 0, stream: int = 0) -> None:
        """Device pointers in and out, asynchronous on `stream` (`epik_amd_placer_place_device`)."""
        capi.check(self._lib.epik_amd_placer_place_device(
            self._handle, d_seqs, d_seq_offsets, int(n), d_rows, d_n_rows, d_kmer_counts or None,
            stream or None))

    # -- strand and frame placement: the same bindings, around their own entry points and mode names --
    @staticmethod
    def _mode(mode, names, what) -> int:
        if isinstance(mode, str):
            if mode not in names:
                raise ValueError(f"unknown {what} {mode!r}: expected one of {sorted(names)}")
            return names[mode]
        return int(mode)

    @staticmethod
    def _strand_mode(mode) -> int:
        return Placer._mode(mode, capi.STRANDS, "strand")

    @staticmethod
    def _frame_mode(mode) -> int:
        return Placer._mode(mode, capi.FRAME_MODES, "translation")

    def _workspace_bytes(self, fn, n: int, seq_bytes: int, mode: int) -> int:
        out = ctypes.c_uint64(0)
        capi.check(fn(self._handle, int(n), int(seq_bytes), mode, ctypes.byref(out)))
        return int(out.value)

    def _place_labelled(self, fn, seqs: np.ndarray, seq_offsets: np.ndarray, mode: int):
        """`place_packed` through a host entry point that also writes a byte per read (strand, frame)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        rows = np.zeros((n, self.keep_at_most), dtype=capi.PLACEMENT)
        n_rows = np.zeros(n, dtype=np.uint32)
        counts = np.zeros((n, self.keep_at_most), dtype=np.uint32)
        label = np.zeros(n, dtype=np.uint8)
        capi.check(fn(self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, mode, rows.ctypes.data,
                      n_rows.ctypes.data, counts.ctypes.data, label.ctypes.data))
        return rows, n_rows, counts, label

    def _place_labelled_device(self, fn, d_seqs, d_seq_offsets, n, mode: int, d_workspace, workspace_bytes, d_rows,
                               d_n_rows, d_kmer_counts, d_label, stream) -> None:
        capi.check(fn(self._handle, d_seqs, d_seq_offsets, int(n), mode, d_workspace or None, int(workspace_bytes),
                      d_rows, d_n_rows, d_kmer_counts or None, d_label or None, stream or None))

    def strand_workspace_bytes(self, n: int, seq_bytes: int, mode="both") -> int:
        """Device workspace `place_strands_device` needs for n reads of seq_bytes characters
        (`epik_amd_placer_strand_workspace_bytes`)."""
        return self._workspace_bytes(self._lib.epik_amd_placer_strand_workspace_bytes, n, seq_bytes,
                                     self._strand_mode(mode))

    def place_strands(self, seqs: np.ndarray, seq_offsets: np.ndarray, mode="both"):
        """`place_packed` on the strand(s) `mode` ("forward" / "reverse" / "both", or capi.STRAND_*) asks for
        (`epik_amd_placer_place_strands`).  Returns (rows, n_rows, kmer_counts, strand[n] uint8: 0 = +, 1 = -)."""
        return self._place_labelled(self._lib.epik_amd_placer_place_strands, seqs, seq_offsets, self._strand_mode(mode))

    def place_strands_device(self, d_seqs: int, d_seq_offsets: int, n: int, mode, d_workspace: int, workspace_bytes: int,
                             d_rows: int, d_n_rows: int, d_kmer_counts: int = 0, d_strand: int = 0,
                             stream: int = 0) -> None:
        """`place_device` on the strand(s) `mode` asks for, asynchronous on `stream`; the caller's workspace of
        `strand_workspace_bytes(n, seq_bytes, mode)` (`epik_amd_placer_place_strands_device`)."""
        self._place_labelled_device(self._lib.epik_amd_placer_place_strands_device, d_seqs, d_seq_offsets, n,
                                    self._strand_mode(mode), d_workspace, workspace_bytes, d_rows, d_n_rows,
                                    d_kmer_counts, d_strand, stream)

    # -- long sequences painted by windows (epik_amd/windows.py) ---------------------------------
    def window_workspace_bytes(self, n: int, num_windows: int, window_bytes: int, mode="forward") -> int:
        """Device workspace `place_windows_device` needs for n reads of num_windows windows and window_bytes window
        characters in total (`epik_amd_placer_window_workspace_bytes`)."""
        out = ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_placer_window_workspace_bytes(self._handle, int(n), int(num_windows), int(window_bytes),
                                                                    self._strand_mode(mode), ctypes.byref(out)))
        return int(out.value)

    def place_windows(self, seqs: np.ndarray, seq_offsets: np.ndarray, window: int, step: int, mode="forward"):
        """Every window of every read placed as a read of its own, on the strand(s) `mode` asks for -- with "both" each
        window picks its strand (`epik_amd_placer_place_windows`).  Returns (rows [V, keep], n_rows [V], kmer_counts
        [V, keep], strand [V] uint8, win_offsets [n + 1] uint64): read i owns the windows win_offsets[i] ..
        win_offsets[i + 1] - 1, V = win_offsets[n]."""
        from . import windows
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        try:
            total = int(windows.win_offsets(np.diff(seq_offsets.astype(np.int64)), int(window), int(step))[-1])
        except ValueError:
            total = 0   # (the library refuses such a window or step, in its own words, before it looks at a buffer)
        rows = np.zeros((total, self.keep_at_most), dtype=capi.PLACEMENT)
        n_rows = np.zeros(total, dtype=np.uint32)
        counts = np.zeros((total, self.keep_at_most), dtype=np.uint32)
        strand = np.zeros(total, dtype=np.uint8)
        win_offs = np.zeros(n + 1, dtype=np.uint64)
        capi.check(self._lib.epik_amd_placer_place_windows(
            self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, int(window), int(step), self._strand_mode(mode),
            rows.ctypes.data, n_rows.ctypes.data, counts.ctypes.data, strand.ctypes.data, win_offs.ctypes.data))
        return rows, n_rows, counts, strand, win_offs

    def place_and_paint_windows(self, seqs: np.ndarray, seq_offsets: np.ndarray, window: int, step: int, group, tau_q: int,
                                mode="forward", rows_out: bool = True):
        """`place_windows` with every chunk's windows painted on the device from the rows the placement left there
        (`epik_amd_placer_paint_windows`): `group` uint32 [num_branches].  `rows_out=False`: rows, row counts and k-mer
        counts stay on the device (None in the result).  Returns (rows, n_rows, kmer_counts, strand, win_offsets,
        records, segments, n_segments)."""
        from . import windows
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        if group.shape != (self.num_branches,):
            raise ValueError(f"group must hold one value per branch ({self.num_branches}), not {group.shape}")
        n = int(seq_offsets.shape[0] - 1)
        try:
            total = int(windows.win_offsets(np.diff(seq_offsets.astype(np.int64)), int(window), int(step))[-1])
        except ValueError:
            total = 0
        rows = np.zeros((total, self.keep_at_most), dtype=capi.PLACEMENT) if rows_out else None
        n_rows = np.zeros(total, dtype=np.uint32) if rows_out else None
        counts = np.zeros((total, self.keep_at_most), dtype=np.uint32) if rows_out else None
        strand, win_offs = np.zeros(total, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
        records, segments = np.zeros(total, dtype=capi.WINDOW_RECORD), np.zeros(total, dtype=capi.WINDOW_SEGMENT)
        n_segments = np.zeros(n, dtype=np.uint32)
        ptr = (lambda a: None if a is None else a.ctypes.data)
        capi.check(self._lib.epik_amd_placer_paint_windows(
            self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, int(window), int(step), self._strand_mode(mode),
            group.ctypes.data, int(tau_q), ptr(rows), ptr(n_rows), ptr(counts), strand.ctypes.data, win_offs.ctypes.data,
            records.ctypes.data, segments.ctypes.data, n_segments.ctypes.data))
        return rows, n_rows, counts, strand, win_offs, records, segments, n_segments

    def place_windows_device(self, d_seqs: int, d_seq_offsets: int, n: int, window: int, step: int, mode, num_windows: int,
                             window_bytes: int, d_workspace: int, workspace_bytes: int, d_rows: int, d_n_rows: int,
                             d_kmer_counts: int = 0, d_strand: int = 0, d_win_offsets: int = 0, stream: int = 0) -> None:
        """`place_windows` on device buffers, asynchronous on `stream`; the caller's totals (epik_amd/windows.py), count
        width (`choose_counts` with min(longest read, window)) and workspace of `window_workspace_bytes`
        (`epik_amd_placer_place_windows_device`)."""
        capi.check(self._lib.epik_amd_placer_place_windows_device(
            self._handle, d_seqs, d_seq_offsets, int(n), int(window), int(step), self._strand_mode(mode), int(num_windows),
            int(window_bytes), d_workspace or None, int(workspace_bytes), d_rows, d_n_rows, d_kmer_counts or None,
            d_strand or None, d_win_offsets or None, stream or None))

    def paint_windows_device(self, d_rows: int, d_n_rows: int, d_kmer_counts: int, d_win_offsets: int, n: int,
                             num_windows: int, d_group: int, tau_q: int, d_records: int = 0, d_segments: int = 0,
                             d_n_segments: int = 0, stream: int = 0, keep: int = None, num_branches: int = None) -> None:
        """The window records, segments and segment counts of the windows whose rows a placement left in device memory,
        asynchronous on `stream` (`epik_amd_windows_paint_device`); `d_group`: uint32 [num_branches].  `keep` and
        `num_branches` default to the placer's (forged rows may have others)."""
        capi.check(self._lib.epik_amd_windows_paint_device(
            self.device, d_rows, d_n_rows, d_kmer_counts, d_win_offsets, int(n), int(num_windows),
            self.keep_at_most if keep is None else int(keep), d_group, self.num_branches if num_branches is None else int(num_branches),
            int(tau_q), d_records or None, d_segments or None, d_n_segments or None, stream or None))

    def paint_windows(self, rows: np.ndarray, n_rows: np.ndarray, kmer_counts: np.ndarray, win_offsets: np.ndarray, group,
                      tau_q: int):
        """`paint_windows_device` for rows that are in host memory (`place_windows`'): copied to the placer's device
        (through torch), painted there and copied back.  Returns (records capi.WINDOW_RECORD [V], segments
        capi.WINDOW_SEGMENT [V] -- read i's at win_offsets[i] + s, the slots beyond n_segments[i] zero --, n_segments [n])."""
        import torch
        dev = torch.device("cuda", self.device)
        rows = np.ascontiguousarray(rows, dtype=capi.PLACEMENT)
        total, keep = rows.shape
        win_offsets = np.ascontiguousarray(win_offsets, dtype=np.uint64)
        group = np.ascontiguousarray(group, dtype=np.uint32)
        n = len(win_offsets) - 1
        if int(win_offsets[-1]) > total or len(n_rows) != total:
            raise ValueError(f"win_offsets name {int(win_offsets[-1])} windows, the rows hold {total}")
        records, segments = np.zeros(total, dtype=capi.WINDOW_RECORD), np.zeros(total, dtype=capi.WINDOW_SEGMENT)
        n_segments = np.zeros(n, dtype=np.uint32)
        if n == 0 or total == 0:
            return records, segments, n_segments
        up = (lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).reshape(-1)).to(dev))
        d_rows, d_n = up(rows, np.float64), up(np.ascontiguousarray(n_rows, dtype=np.uint32), np.int32)
        d_counts = up(np.ascontiguousarray(kmer_counts, dtype=np.uint32), np.int32)
        d_wo, d_group = up(win_offsets, np.int64), up(group, np.int32)
        d_rec = torch.zeros(total * 4, dtype=torch.int32, device=dev)
        d_seg = torch.zeros(total * 4, dtype=torch.int64, device=dev)
        d_ns = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        self.paint_windows_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_wo.data_ptr(), n, int(win_offsets[-1]),
                                  d_group.data_ptr(), tau_q, d_rec.data_ptr(), d_seg.data_ptr(), d_ns.data_ptr(), keep=keep,
                                  num_branches=len(group))
        torch.cuda.synchronize(dev)
        records[:] = d_rec.cpu().numpy().view(capi.WINDOW_RECORD)
        segments[:] = d_seg.cpu().numpy().view(capi.WINDOW_SEGMENT)
        n_segments[:] = d_ns.cpu().numpy().view(np.uint32)
        return records, segments, n_segments

    # -- paired-end reads, one placement per fragment ---------------------------------------------
    @staticmethod
    def _mates_mode(strand, orientation) -> int:
        return Placer._strand_mode(strand) | Placer._mode(orientation, capi.MATE_ORIENTATIONS, "mate orientation")

    def mates_separator(self) -> int:
        """The byte the library puts between the mates of a pair (`epik_amd_placer_mates_separator`)."""
        out = ctypes.c_uint8(0)
        capi.check(self._lib.epik_amd_placer_mates_separator(self._handle, ctypes.byref(out)))
        return int(out.value)

    def mates_workspace_bytes(self, n_pairs: int, seq_bytes: int, strand="forward", orientation="fr") -> int:
        """Device workspace `place_mates_device` needs for n_pairs pairs of seq_bytes characters in total
        (`epik_amd_placer_mates_workspace_bytes`)."""
        return self._workspace_bytes(self._lib.epik_amd_placer_mates_workspace_bytes, n_pairs, seq_bytes,
                                     self._mates_mode(strand, orientation))

    @staticmethod
    def _pairs_of(seq_offsets: np.ndarray) -> int:
        if seq_offsets.shape[0] % 2 != 1:
            raise ValueError("an interleaved batch of pairs has an even number of reads (2 n + 1 offsets)")
        return int(seq_offsets.shape[0] - 1) // 2

    def place_mates(self, seqs: np.ndarray, seq_offsets: np.ndarray, strand="forward", orientation="fr"):
        """One placement per pair of ONE interleaved batch -- read 2 i is mate 1, read 2 i + 1 mate 2 of pair i --: the
        placement of mate 1 . separator . rc(mate 2) ("fr") or mate 1 . separator . mate 2 ("ff"), on the strand(s)
        `strand` asks for (`epik_amd_placer_place_mates`).  Returns (rows, n_rows, kmer_counts, strand[n] uint8), all
        per pair."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = self._pairs_of(seq_offsets)
        rows = np.zeros((n, self.keep_at_most), dtype=capi.PLACEMENT)
        n_rows = np.zeros(n, dtype=np.uint32)
        counts = np.zeros((n, self.keep_at_most), dtype=np.uint32)
        label = np.zeros(n, dtype=np.uint8)
        capi.check(self._lib.epik_amd_placer_place_mates(
            self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, self._mates_mode(strand, orientation),
            rows.ctypes.data, n_rows.ctypes.data, counts.ctypes.data, label.ctypes.data))
        return rows, n_rows, counts, label

    def place_mates_device(self, d_seqs: int, d_seq_offsets: int, n_pairs: int, seq_bytes: int, strand, orientation,
                           d_workspace: int, workspace_bytes: int, d_rows: int, d_n_rows: int, d_kmer_counts: int = 0,
                           d_strand: int = 0, stream: int = 0) -> None:
        """`place_mates` on device buffers, asynchronous on `stream`; the caller's workspace of
        `mates_workspace_bytes(n_pairs, seq_bytes, ...)` and count width (`choose_counts` with the longest joined
        sequence, len1 + len2 + 1) (`epik_amd_placer_place_mates_device`)."""
        capi.check(self._lib.epik_amd_placer_place_mates_device(
            self._handle, d_seqs, d_seq_offsets, int(n_pairs), int(seq_bytes), self._mates_mode(strand, orientation),
            d_workspace or None, int(workspace_bytes), d_rows, d_n_rows, d_kmer_counts or None, d_strand or None,
            stream or None))

    # -- the abundance profile (epik_amd/profile.py) ----------------------------------------------
    def profile(self):
        """A new, empty device profile for this placer (`epik_amd_profile_create`)."""
        from .profile import Profile
        return Profile(self)

    def profile_packed(self, profile, seqs: np.ndarray, seq_offsets: np.ndarray, weights=None, strand=None, translate=None,
                       mates=None):
        """`place_packed` / `place_strands` / `place_frames` / `place_mates` with the rows left on the device and added
        to `profile` there, read i with weights[i] (None: 1): `epik_amd_placer_profile_reads` / `_strands` / `_frames`
        / `_mates`.  `mates` ("fr" / "ff"): the batch is interleaved pairs, counted and weighted per pair.  Returns
        the strand or frame byte per read or pair (None without `strand`, `translate` and `mates`)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        if strand is not None and translate is not None:
            raise ValueError("strand and translate do not combine: translate=both already covers both strands")
        if mates is not None:
            if translate is not None:
                raise ValueError("mates and translate do not combine: pairs are placed on nucleotide databases")
            n = self._pairs_of(seq_offsets)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
        if w is not None and w.shape != (n,):
            raise ValueError(f"weights must hold one value per read ({n}), not {w.shape}")
        w_ptr = None if w is None else w.ctypes.data
        if strand is None and translate is None and mates is None:
            capi.check(self._lib.epik_amd_placer_profile_reads(self._handle, profile._handle, seqs.ctypes.data,
                                                               seq_offsets.ctypes.data, w_ptr, n))
            return None
        label = np.zeros(n, dtype=np.uint8)
        if mates is not None:
            fn, mode = self._lib.epik_amd_placer_profile_mates, self._mates_mode(strand or "forward", mates)
        elif translate is not None:
            fn, mode = self._lib.epik_amd_placer_profile_frames, self._frame_mode(translate)
        else:
            fn, mode = self._lib.epik_amd_placer_profile_strands, self._strand_mode(strand)
        capi.check(fn(self._handle, profile._handle, seqs.ctypes.data, seq_offsets.ctypes.data, w_ptr, n, mode,
                      label.ctypes.data))
        return label

    # -- a cohort of samples (epik_amd/cohort.py) -------------------------------------------------
    def cohort(self, num_samples: int):
        """A new, empty device cohort of `num_samples` samples for this placer (`epik_amd_cohort_create`)."""
        from .cohort import Cohort
        return Cohort(self, num_samples)

    def cohort_packed(self, cohort, seqs: np.ndarray, seq_offsets: np.ndarray, samples, weights=None, strand=None,
                      translate=None, mates=None):
        """`profile_packed` with read (or pair) i added to row samples[i] of `cohort`: `epik_amd_placer_cohort_reads` /
        `_strands` / `_frames` / `_mates`.  Returns the strand or frame byte per read or pair (None without `strand`,
        `translate` and `mates`)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        if strand is not None and translate is not None:
            raise ValueError("strand and translate do not combine: translate=both already covers both strands")
        if mates is not None:
            if translate is not None:
                raise ValueError("mates and translate do not combine: pairs are placed on nucleotide databases")
            n = self._pairs_of(seq_offsets)
        smp = np.ascontiguousarray(samples, dtype=np.uint32)
        if smp.shape != (n,):
            raise ValueError(f"samples must hold one value per read ({n}), not {smp.shape}")
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
        if w is not None and w.shape != (n,):
            raise ValueError(f"weights must hold one value per read ({n}), not {w.shape}")
        w_ptr = None if w is None else w.ctypes.data
        if strand is None and translate is None and mates is None:
            capi.check(self._lib.epik_amd_placer_cohort_reads(self._handle, cohort._handle, seqs.ctypes.data,
                                                              seq_offsets.ctypes.data, w_ptr, smp.ctypes.data, n))
            return None
        label = np.zeros(n, dtype=np.uint8)
        if mates is not None:
            fn, mode = self._lib.epik_amd_placer_cohort_mates, self._mates_mode(strand or "forward", mates)
        elif translate is not None:
            fn, mode = self._lib.epik_amd_placer_cohort_frames, self._frame_mode(translate)
        else:
            fn, mode = self._lib.epik_amd_placer_cohort_strands, self._strand_mode(strand)
        capi.check(fn(self._handle, cohort._handle, seqs.ctypes.data, seq_offsets.ctypes.data, w_ptr, smp.ctypes.data, n,
                      mode, label.ctypes.data))
        return label

    # -- taxonomic assignment (epik_amd/taxonomy.py) -------------------------------------------
    def taxonomy(self, taxon_parent, label, num_samples: int = 1):
        """A new, empty device taxonomy object for this placer (`epik_amd_taxonomy_create`): `taxon_parent[t]` of every
        taxon (post-order ids; the root's: -1 or capi.TREE_NO_PARENT), `label[b]` of every branch."""
        from .taxonomy import DeviceTaxonomy
        return DeviceTaxonomy(self, taxon_parent, label, num_samples)

    def taxa_packed(self, taxonomy, seqs: np.ndarray, seq_offsets: np.ndarray, tau_q: int, weights=None, samples=None,
                    profile=None, cohort=None, strand=None, translate=None, mates=None, rows_out: bool = True,
                    records_out: bool = True):
        """`place_packed` / `place_strands` / `place_frames` / `place_mates` with every read's (or pair's) rows added to
        the device `taxonomy` object there: `epik_amd_placer_taxa_reads` / `_strands` / `_frames` / `_mates`.  Item i
        counts weights[i] times (None: once) for row samples[i] (None: row 0); `profile` or `cohort` (not both): the
        rows are also added to it.  `rows_out=False`: rows, row counts and k-mer counts stay on the device;
        `records_out=False`: no record is computed.  Returns (rows, n_rows, kmer_counts, label, records)."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        if strand is not None and translate is not None:
            raise ValueError("strand and translate do not combine: translate=both already covers both strands")
        if mates is not None:
            if translate is not None:
                raise ValueError("mates and translate do not combine: pairs are placed on nucleotide databases")
            n = self._pairs_of(seq_offsets)
        per_item = []
        for what, a in (("weights", weights), ("samples", samples)):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
            if a is not None and a.shape != (n,):
                raise ValueError(f"{what} must hold one value per read ({n}), not {a.shape}")
            per_item.append(a)
        rows = np.zeros((n, self.keep_at_most), dtype=capi.PLACEMENT) if rows_out else None
        n_rows = np.zeros(n, dtype=np.uint32) if rows_out else None
        counts = np.zeros((n, self.keep_at_most), dtype=np.uint32) if rows_out else None
        records = np.zeros(n, dtype=capi.TAXON_RECORD) if records_out else None
        ptr = (lambda a: None if a is None else a.ctypes.data)
        out = [ptr(a) for a in (rows, n_rows, counts)]
        tail = [taxonomy._handle, int(tau_q), ptr(records), ptr(per_item[0]), ptr(per_item[1]),
                None if profile is None else profile._handle, None if cohort is None else cohort._handle]
        if strand is None and translate is None and mates is None:
            capi.check(self._lib.epik_amd_placer_taxa_reads(self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, *out, *tail))
            return rows, n_rows, counts, None, records
        label = np.zeros(n, dtype=np.uint8)
        if mates is not None:
            fn, mode = self._lib.epik_amd_placer_taxa_mates, self._mates_mode(strand or "forward", mates)
        elif translate is not None:
            fn, mode = self._lib.epik_amd_placer_taxa_frames, self._frame_mode(translate)
        else:
            fn, mode = self._lib.epik_amd_placer_taxa_strands, self._strand_mode(strand)
        capi.check(fn(self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, mode, *out, label.ctypes.data, *tail))
        return rows, n_rows, counts, label, records

    # -- placement confidence (epik_amd/confidence.py) ------------------------------------------
    def tree(self, parent, branch_length):
        """The tree of this placer's database on its device (`epik_amd_tree_create`): `parent[b]` of every post-order
        id (the root's: -1 or capi.TREE_NO_PARENT) and the branch lengths."""
        from .confidence import Tree
        if len(parent) != self.num_branches:
            raise ValueError(f"the tree has {len(parent)} branches, the placer {self.num_branches}")
        return Tree(self.device, parent, branch_length)

    def confidence_device(self, tree, d_rows: int, d_n_rows: int, d_kmer_counts: int, n: int, tau_q: int, d_out: int,
                          stream: int = 0) -> None:
        """The confidence records of the n reads whose rows a placement of this placer left in device memory, into
        d_out (16 bytes a read), asynchronous on `stream` (`epik_amd_confidence_device`)."""
        tree.confidence_device(d_rows, d_n_rows, d_kmer_counts, n, self.keep_at_most, tau_q, d_out, stream)

    def confidence_packed(self, tree, seqs: np.ndarray, seq_offsets: np.ndarray, tau_q: int, profile=None, weights=None,
                          strand=None, translate=None, mates=None, rows_out: bool = True):
        """`place_packed` / `place_strands` / `place_frames` / `place_mates` with the confidence record of every read or
        pair computed on the device from its rows: `epik_amd_placer_confidence_reads` / `_strands` / `_frames` /
        `_mates`.  `profile`: the rows are also added to it there, item i with weights[i] (None: 1).  `rows_out=False`:
        rows, row counts and k-mer counts stay on the device (None in the result).  Returns (rows, n_rows, kmer_counts,
        label, conf): label the strand or frame byte per item (None without `strand`, `translate` and `mates`), conf
        capi.CONFIDENCE records."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        if strand is not None and translate is not None:
            raise ValueError("strand and translate do not combine: translate=both already covers both strands")
        if mates is not None:
            if translate is not None:
                raise ValueError("mates and translate do not combine: pairs are placed on nucleotide databases")
            n = self._pairs_of(seq_offsets)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
        if w is not None and w.shape != (n,):
            raise ValueError(f"weights must hold one value per read ({n}), not {w.shape}")
        rows = np.zeros((n, self.keep_at_most), dtype=capi.PLACEMENT) if rows_out else None
        n_rows = np.zeros(n, dtype=np.uint32) if rows_out else None
        counts = np.zeros((n, self.keep_at_most), dtype=np.uint32) if rows_out else None
        conf = np.zeros(n, dtype=capi.CONFIDENCE)
        out = [None if a is None else a.ctypes.data for a in (rows, n_rows, counts)]
        tail = [tree._handle, int(tau_q), conf.ctypes.data, None if profile is None else profile._handle,
                None if w is None else w.ctypes.data]
        if strand is None and translate is None and mates is None:
            capi.check(self._lib.epik_amd_placer_confidence_reads(self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n,
                                                                  *out, *tail))
            return rows, n_rows, counts, None, conf
        label = np.zeros(n, dtype=np.uint8)
        if mates is not None:
            fn, mode = self._lib.epik_amd_placer_confidence_mates, self._mates_mode(strand or "forward", mates)
        elif translate is not None:
            fn, mode = self._lib.epik_amd_placer_confidence_frames, self._frame_mode(translate)
        else:
            fn, mode = self._lib.epik_amd_placer_confidence_strands, self._strand_mode(strand)
        capi.check(fn(self._handle, seqs.ctypes.data, seq_offsets.ctypes.data, n, mode, *out, label.ctypes.data, *tail))
        return rows, n_rows, counts, label, conf

    @staticmethod
    def codon_table() -> np.ndarray:
        """The library's codon -> residue table: uint8[4096] indexed by the three nucleotide class masks, 4 bits each,
        first nucleotide most significant (`epik_amd_codon_table`; needs no device)."""
        out = np.zeros(4096, dtype=np.uint8)
        capi.check(capi.load().epik_amd_codon_table(out.ctypes.data))
        return out

    def frame_workspace_bytes(self, n: int, seq_bytes: int, mode="both") -> int:
        """Device workspace `place_frames_device` needs for n nucleotide reads of seq_bytes characters
        (`epik_amd_placer_frame_workspace_bytes`)."""
        return self._workspace_bytes(self._lib.epik_amd_placer_frame_workspace_bytes, n, seq_bytes,
                                     self._frame_mode(mode))

    def place_frames(self, seqs: np.ndarray, seq_offsets: np.ndarray, mode="both"):
        """`place_packed` for nucleotide reads on this amino-acid database, through the frames `mode` ("forward" /
        "reverse" / "both", or capi.FRAMES_*) asks for; per read the best frame (`epik_amd_placer_place_frames`).
        Returns (rows, n_rows, kmer_counts, frame[n] uint8: 0..5 = +1 +2 +3 -1 -2 -3)."""
        return self._place_labelled(self._lib.epik_amd_placer_place_frames, seqs, seq_offsets, self._frame_mode(mode))

    def place_frames_device(self, d_seqs: int, d_seq_offsets: int, n: int, mode, d_workspace: int,
                            workspace_bytes: int, d_rows: int, d_n_rows: int, d_kmer_counts: int = 0,
                            d_frame: int = 0, stream: int = 0) -> None:
        """`place_frames` on device buffers, asynchronous on `stream`; the caller's workspace of
        `frame_workspace_bytes(n, seq_bytes, mode)` and count width (`choose_counts` with the longest frame,
        L // 3) (`epik_amd_placer_place_frames_device`)."""
        self._place_labelled_device(self._lib.epik_amd_placer_place_frames_device, d_seqs, d_seq_offsets, n,
                                    self._frame_mode(mode), d_workspace, workspace_bytes, d_rows, d_n_rows,
                                    d_kmer_counts, d_frame, stream)

    def accumulate_device(self, d_seqs: int, d_seq_offsets: int, n: int, d_scores: int, d_counts: int,
                          stream: int = 0, d_amb_slot: int = 0, d_amb_order: int = 0, d_amb_avg: int = 0) -> None:
        """First half of a k-mer-space-sharded placement: raw float32 score sums and uint16 k-mer counts
        of this shard's lists, [n][num_branches] each, and -- for the reads with a slot in d_amb_slot --
        the records of their ambiguous k-mers (`epik_amd_placer_accumulate_device`)."""
        capi.check(self._lib.epik_amd_placer_accumulate_device(
            self._handle, d_seqs, d_seq_offsets, int(n), d_scores, d_counts, d_amb_slot or None,
            d_amb_order or None, d_amb_avg or None, stream or None))

    def finish_device(self, d_seq_offsets: int, n: int, d_scores: int, d_counts: int, d_rows: int,
                      d_n_rows: int, d_kmer_counts: int = 0, stream: int = 0, d_amb_slot: int = 0,
                      d_amb_avg: int = 0) -> None:
        """Second half: correction, top-k and like-weight-ratio on the sums added over the shards
        (`epik_amd_placer_finish_device`)."""
        capi.check(self._lib.epik_amd_placer_finish_device(
            self._handle, d_seq_offsets, int(n), d_scores, d_counts, d_amb_slot or None, d_amb_avg or None,
            d_rows, d_n_rows, d_kmer_counts or None, stream or None))

    def partial_info(self) -> dict:
        """Geometry of the partial lists of this handle (`epik_amd_placer_partial_info`)."""
        info = capi.PartialInfo()
        capi.check(self._lib.epik_amd_placer_partial_info(self._handle, ctypes.byref(info)))
        return {"lists": bool(info.lists), "slices": int(info.slices), "slice_rows": int(info.slice_rows),
                "entry_bytes": int(info.entry_bytes), "num_branches": int(info.num_branches),
                "postings_per_kmer": float(info.postings_per_kmer)}

    def accumulate_lists_device(self, d_seqs: int, d_seq_offsets: int, n: int, n_parts: int, d_entries: int,
                                entries_cap: int, d_index: int, d_part_entries: int, stream: int = 0,
                                d_amb_slot: int = 0, d_amb_order: int = 0, d_amb_avg: int = 0) -> None:
        """First half of a k-mer-space-sharded placement with partial LISTS: per read and slice of the branch
        range only the rows this shard's lists touched (`epik_amd_placer_accumulate_lists_device`)."""
        capi.check(self._lib.epik_amd_placer_accumulate_lists_device(
            self._handle, d_seqs, d_seq_offsets, int(n), int(n_parts), d_entries or None, int(entries_cap), d_index,
            d_part_entries, d_amb_slot or None, d_amb_order or None, d_amb_avg or None, stream or None))

    def finish_lists_device(self, d_seq_offsets: int, n: int, d_entries, d_index, d_rows: int, d_n_rows: int,
                            d_kmer_counts: int = 0, stream: int = 0, d_amb_slot: int = 0, d_amb_avg: int = 0) -> None:
        """Second half: the shards' lists of the n reads (d_entries[g], d_index[g]: device addresses, one per
        shard, in shard order) added in that order, then correction, top-k and like-weight-ratio
        (`epik_amd_placer_finish_lists_device`)."""
        g = len(d_entries)
        assert len(d_index) == g
        entries = (ctypes.c_void_p * g)(*[int(x) or None for x in d_entries])
        index = (ctypes.c_void_p * g)(*[int(x) or None for x in d_index])
        capi.check(self._lib.epik_amd_placer_finish_lists_device(
            self._handle, d_seq_offsets, int(n), g, entries, index, d_amb_slot or None, d_amb_avg or None,
            d_rows, d_n_rows, d_kmer_counts or None, stream or None))

    @staticmethod
    def place_sharded(placers, seqs: np.ndarray, seq_offsets: np.ndarray):
        """`epik_amd_placer_place_sharded`: host reads placed on `placers`, handle g holding shard g of
        len(placers) of one database (any devices).  Returns like `place_packed`."""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        seq_offsets = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = int(seq_offsets.shape[0] - 1)
        keep = placers[0].keep_at_most
        rows = np.zeros((n, keep), dtype=capi.PLACEMENT)
        n_rows = np.zeros(n, dtype=np.uint32)
        counts = np.zeros((n, keep), dtype=np.uint32)
        handles = (ctypes.c_void_p * len(placers))(*[p._handle for p in placers])
        capi.check(placers[0]._lib.epik_amd_placer_place_sharded(
            handles, len(placers), seqs.ctypes.data, seq_offsets.ctypes.data, n, rows.ctypes.data, n_rows.ctypes.data,
            counts.ctypes.data))
        return rows, n_rows, counts

    def release_scratch(self) -> None:
        """Frees what the handle's launches have grown and kept (`epik_amd_placer_release_scratch`)."""
        capi.check(self._lib.epik_amd_placer_release_scratch(self._handle))

    def last_path(self) -> int:
        """Which kernels the last launch ran: capi.PATH_WAVE / PATH_TEAM_ONE_KERNEL / PATH_TEAM_STREAMED."""
        out = ctypes.c_uint32(0)
        capi.check(self._lib.epik_amd_placer_last_path(self._handle, ctypes.byref(out)))
        return int(out.value)

    def stream_build(self) -> dict:
        """Which build of the streaming kernel a large-tree placer launches with its current count width, and how many
        touched quads an item may have to take the touched-quad epilogue (`epik_amd_placer_stream_build`)."""
        wide, quads = ctypes.c_uint32(0), ctypes.c_uint32(0)
        capi.check(self._lib.epik_amd_placer_stream_build(self._handle, ctypes.byref(wide), ctypes.byref(quads)))
        return {"wide": bool(wide.value), "sparse_quads": int(quads.value)}

    def choose_counts(self, longest_read: int) -> None:
        """Width of the per-branch counts for the device entry points, chosen as `place_packed`
        chooses it from the batch (`epik_amd_placer_choose_counts`)."""
        capi.check(self._lib.epik_amd_placer_choose_counts(self._handle, int(longest_read)))

    def algorithmic_bytes(self, d_seqs: int, d_seq_offsets: int, n: int, d_n_rows: int = 0,
                          stream: int = 0) -> int:
        out = ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_placer_algorithmic_bytes(
            self._handle, d_seqs, d_seq_offsets, int(n), d_n_rows or None, stream or None,
            ctypes.byref(out)))
        return int(out.value)

    def launch_info(self) -> dict:
        w, b, l = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        capi.check(self._lib.epik_amd_placer_launch_info(self._handle, ctypes.byref(w),
                                                         ctypes.byref(b), ctypes.byref(l)))
        return {"waves_per_block": w.value, "blocks": b.value, "lds_bytes_per_block": l.value}

    def set_timing(self, enabled: bool) -> None:
        capi.check(self._lib.epik_amd_placer_set_timing(self._handle, int(bool(enabled))))

    def last_kernel_ms(self) -> float:
        ms = ctypes.c_float(-1.0)
        capi.check(self._lib.epik_amd_placer_last_kernel_ms(self._handle, ctypes.byref(ms)))
        return float(ms.value)

    # -- epik::placer::place ---------------------------------------------------------
    def place(self, seq_records: Iterable[Tuple[str, str]], num_threads: int = 1,
              strand: str = "forward", translate=None, profile=None, mates=None,
              mate_orientation: str = "fr", assign=None, tree=None) -> PlacedCollection:
        """`seq_records` = (header, sequence) pairs (i2l::seq_record).  `num_threads`
        is accepted for signature parity and ignored, as the parallelism is the GPU's.
        `strand`: "forward" (the reference's contract: each read as given), "reverse" (its reverse
        complement) or "both" (per read the better of the two; PlacedSequence.strand says which).
        `translate` (amino-acid databases): None places the reads as given; "forward" / "reverse" / "both" takes
        them as nucleotide reads and places their frames +1 +2 +3 / -1 -2 -3 / all six, per read the best one
        (PlacedSequence.frame says which).  Duplicates are merged on the nucleotide string.
        `profile` (a `Profile` of this placer): the placements are also added to it, every unique sequence with the
        number of its records as weight.
        `mates` (nucleotide databases): the second mates, (header, sequence) records in the order of `seq_records`;
        every pair gets ONE placement, that of mate 1 . separator . rc(mate 2) (`mate_orientation` "fr") or mate 1 .
        separator . mate 2 ("ff") (`place_mates`).  Duplicates are merged on the PAIR of sequences: `sequence_map` is
        then keyed by (mate 1, mate 2) and holds mate 1's headers; PlacedSequence.sequence is mate 1, .mate mate 2,
        .strand the fragment's strand.
        `assign` (a mass tau in [0, 1]) with `tree` (a `Tree` of this placer, `Placer.tree`): the placement goes through
        the confidence entries and PlacedCollection.confidence holds, per placed sequence, the LCA clade that holds
        tau of its placement mass, that clade's mass and the EDPL, computed on the device."""
        del num_threads
        if (assign is None) != (tree is None):
            raise ValueError("assign (the mass tau) and tree (Placer.tree(...)) go together")
        mode = self._strand_mode(strand)
        frame_mode = None if translate is None else self._frame_mode(translate)
        if frame_mode is not None and mode != capi.STRAND_FORWARD:
            raise ValueError("strand and translate do not combine: translate=both already covers both strands")
        if mates is not None and frame_mode is not None:
            raise ValueError("mates and translate do not combine: pairs are placed on nucleotide databases")
        sequence_map: dict = {}
        if mates is not None:
            seq_records, mates = list(seq_records), list(mates)
            check_mate_names([h for h, _ in seq_records], [h for h, _ in mates])
            for (header, sequence), (_, mate) in zip(seq_records, mates):
                sequence_map.setdefault((sequence, mate), []).append(header)
        else:
            for header, sequence in seq_records:          # place.cpp:73-81
                sequence_map.setdefault(sequence, []).append(header)
        unique = list(sequence_map.keys())            # place.cpp:52-63
        bufs = [s.encode() for s in unique] if mates is None else [m.encode() for pair in unique for m in pair]
        offsets = np.zeros(len(bufs) + 1, dtype=np.uint64)
        if bufs:
            offsets[1:] = np.cumsum([len(b) for b in bufs], dtype=np.uint64)
        data = np.frombuffer(b"".join(bufs), dtype=np.uint8) if bufs else np.zeros(0, np.uint8)
        strands = frames = conf = None
        if assign is not None:
            from .confidence import tau_q
            rows, n_rows, counts, label, conf = self.confidence_packed(
                tree, data, offsets, tau_q(assign), strand=None if frame_mode is not None or (mates is None and mode == capi.STRAND_FORWARD) else mode,
                translate=frame_mode, mates=None if mates is None else mate_orientation)
            if frame_mode is not None:
                frames = label
            elif mates is not None or mode != capi.STRAND_FORWARD:
                strands = label
        elif mates is not None:
            rows, n_rows, counts, strands = self.place_mates(data, offsets, mode, mate_orientation)
        elif frame_mode is not None:
            rows, n_rows, counts, frames = self.place_frames(data, offsets, frame_mode)
        elif mode == capi.STRAND_FORWARD:
            rows, n_rows, counts = self.place_packed(data, offsets)
        else:
            rows, n_rows, counts, strands = self.place_strands(data, offsets, mode)
        if profile is not None:
            profile.add_host(rows, n_rows, counts, [len(sequence_map[s]) for s in unique])
        if len(n_rows) and int(n_rows.max()) > self.keep_at_most:
            # (never from place_packed, which widens the counts by itself: a row count, not the
            # EPIK_AMD_ROWS_COUNTS_TOO_NARROW mark of the device entry points)
            raise RuntimeError(f"a read came back with {int(n_rows.max())} rows (keep_at_most {self.keep_at_most})")
        placed = []
        for i, seq in enumerate(unique):
            pl = []
            for r in range(int(n_rows[i])):
                b = int(rows[i, r]["branch"])
                in_tree = self.distal is not None and b < self.num_branches
                pl.append(Placement(
                    branch_id=b, score=float(rows[i, r]["score"]),
                    weight_ratio=float(rows[i, r]["lwr"]), count=int(counts[i, r]),
                    # rows fabricated for a read without hits carry 0.0 lengths (place.cpp:150)
                    distal_length=float(self.distal[b]) if in_tree and counts[i, r] else 0.0,
                    pendant_length=float(self.pendant[b]) if in_tree and counts[i, r] else 0.0))
            seq, mate = seq if mates is not None else (seq, None)
            placed.append(PlacedSequence(sequence=seq, placements=pl, mate=mate,
                                         strand="-" if strands is not None and strands[i] else "+",
                                         frame=capi.FRAME_NAMES[int(frames[i])] if frames is not None else ""))
        return PlacedCollection(sequence_map=sequence_map, placed_seqs=placed, confidence=conf)
