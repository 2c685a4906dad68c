"""Long sequences painted by windows (include/epik_amd.h: epik_amd_window_span, epik_amd_windows_paint_*): the window
geometry, the rule of the records and the segments over whole arrays (`numpy_paint`), worded after the header, the
same rule on the host through the library (`paint_host`), the breakpoints between called segments, and the files."""
from __future__ import annotations

import numpy as np

from . import capi

LWR_BITS = capi.PROFILE_LWR_BITS
U64 = np.uint64
CALLED_BELOW = capi.WINDOW_AMBIGUOUS      # a call below this is a group


def tau_q_of(share: float) -> int:
    """--window-mass as the rule takes it: llrint(share * 2^30), share in (0.5, 1]; the result lies in (2^29, 2^30]."""
    share = float(share)
    tq = int(np.rint(np.float64(share) * np.float64(1 << LWR_BITS))) if 0.0 <= share <= 1.0 else 0
    if not (1 << (LWR_BITS - 1)) < tq <= (1 << LWR_BITS):
        raise ValueError(f"the window mass must lie in (0.5, 1], not {share}")
    return tq


def _check(window: int, step: int) -> None:
    if not (0 < window < (1 << 31) and 1 <= step <= window):
        raise ValueError(f"window {window}, step {step}: 0 < window < 2^31 and 1 <= step <= window")


def window_count(length: int, window: int, step: int) -> int:
    """The windows of a read of `length` characters: 1 up to `window` characters, else 1 + ceil((L - W) / S)."""
    _check(window, step)
    return 1 if length <= window else 1 + (length - window + step - 1) // step


def window_span(length: int, window: int, step: int, w: int):
    """Window w of such a read, 0-based half-open: [w S, w S + W), the last one [L - W, L); [0, L) for L <= W."""
    nw = window_count(length, window, step)
    if not 0 <= w < nw:
        raise IndexError(f"window {w} of {nw}")
    if length <= window:
        return 0, length
    begin = w * step if w + 1 < nw else length - window
    return begin, begin + window


def win_offsets(lengths, window: int, step: int) -> np.ndarray:
    """win_offsets[n + 1] (uint64) of a batch of reads of these lengths: the exclusive sum of their windows."""
    _check(window, step)
    lengths = np.asarray(lengths).astype(np.int64)
    nw = np.where(lengths <= window, 1, 1 + (np.maximum(lengths - window, 0) + step - 1) // step)
    return np.concatenate([[0], np.cumsum(nw)]).astype(U64)


def slice_windows(seqs, seq_offsets, window: int, step: int):
    """The windows of a packed batch cut on the host: (bytes, offsets [num_windows + 1], win_offsets [n + 1])."""
    seqs = np.asarray(seqs, dtype=np.uint8)
    offs = np.asarray(seq_offsets).astype(np.int64)
    parts, lens = [], []
    for i in range(len(offs) - 1):
        length = int(offs[i + 1] - offs[i])
        for w in range(window_count(length, window, step)):
            b, e = window_span(length, window, step, w)
            parts.append(seqs[offs[i] + b:offs[i] + e])
            lens.append(e - b)
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return data, np.concatenate([[0], np.cumsum(lens)]).astype(U64), win_offsets(np.diff(offs), window, step)


def numpy_paint(rows, n_rows, counts, win_offs, group, tau_q):
    """The records (capi.WINDOW_RECORD [V]), the segments (capi.WINDOW_SEGMENT [V], read i's at win_offs[i] + s, the
    slots beyond n_segments[i] zero) and n_segments [n] of the rule of include/epik_amd.h.  The mass of every group a
    window's rows name is summed; the one comparison a window needs is made on Python ints."""
    group = np.asarray(group).astype(np.int64)
    N = len(group)
    V, keep = rows.shape
    tau_q = int(tau_q)
    assert (1 << (LWR_BITS - 1)) < tau_q <= (1 << LWR_BITS)
    n_rows = np.asarray(n_rows).astype(np.int64)
    call = np.zeros(V, np.int64)
    call[n_rows == capi.ROWS_COUNTS_TOO_NARROW] = capi.WINDOW_TOO_NARROW
    call[(call == 0) & (n_rows == 0)] = capi.WINDOW_TOO_SHORT
    call[(call == 0) & (np.asarray(counts).reshape(V, keep)[:, 0] == 0)] = capi.WINDOW_NO_HIT
    live = np.where(call != 0, 0, np.minimum(n_rows, keep))
    slot = np.arange(keep)[None, :] < live[:, None]
    branch = rows["branch"].astype(np.int64)
    call[(slot & (branch >= N)).any(axis=1)] = capi.WINDOW_BAD_ROW
    mine = slot & (call == 0)[:, None]
    g = np.where(mine, group[np.where(mine, branch, 0)], capi.WINDOW_NO_GROUP)
    q = np.rint(np.where(mine, rows["lwr"], 0.0) * np.float64(1 << LWR_BITS)).astype(np.int64).astype(U64)
    total = q.sum(axis=1, dtype=U64)
    call[(call == 0) & (total == 0)] = capi.WINDOW_NO_MASS
    mass = np.zeros(V, U64)
    for lo in range(0, V, 512):
        sl = slice(lo, min(lo + 512, V))
        same = (g[sl][:, :, None] == g[sl][:, None, :]) & (g[sl] != capi.WINDOW_NO_GROUP)[:, :, None]
        m = (same * q[sl][:, None, :]).sum(axis=2, dtype=U64)            # of the group of every row
        best = m.argmax(axis=1)
        for v in np.flatnonzero(call[sl] == 0):
            mv = int(m[v, best[v]])
            if mv and (mv << LWR_BITS) >= tau_q * int(total[lo + v]):
                call[lo + v], mass[lo + v] = g[lo + v, best[v]], mv
            else:
                call[lo + v] = capi.WINDOW_AMBIGUOUS
    called = call < CALLED_BELOW
    mass, total = np.where(called, mass, U64(0)), np.where(called, total, U64(0))
    records = np.zeros(V, dtype=capi.WINDOW_RECORD)
    records["call"] = call
    records["call_mass_q"] = np.minimum(mass, U64(0xFFFFFFFF))
    records["first_group"] = np.where(called, g[:, 0], 0) if keep else 0
    records["total_q"] = np.minimum(total, U64(0xFFFFFFFF))

    win_offs = np.asarray(win_offs).astype(np.int64)
    n = len(win_offs) - 1
    segments, n_segments = np.zeros(V, dtype=capi.WINDOW_SEGMENT), np.zeros(n, np.uint32)
    for i in range(n):
        v0, v1 = win_offs[i], win_offs[i + 1]
        if v1 <= v0:
            continue
        c = call[v0:v1]
        heads = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
        ends = np.append(heads[1:], v1 - v0)
        seg = segments[v0:v0 + len(heads)]
        seg["call"], seg["first_window"], seg["num_windows"] = c[heads], heads, ends - heads
        seg["call_mass"] = np.add.reduceat(mass[v0:v1], heads)
        seg["total"] = np.add.reduceat(total[v0:v1], heads)
        n_segments[i] = len(heads)
    return records, segments, n_segments


def paint_host(rows, n_rows, counts, win_offs, group, tau_q):
    """The rule on the host through the library (`epik_amd_windows_paint_host`): (records, segments, n_segments)."""
    lib = capi.load()
    rows = np.ascontiguousarray(rows, dtype=capi.PLACEMENT)
    V, keep = rows.shape
    n_rows = np.ascontiguousarray(n_rows, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    win_offs = np.ascontiguousarray(win_offs, dtype=U64)
    group = np.ascontiguousarray(group, dtype=np.uint32)
    n = len(win_offs) - 1
    if n_rows.shape != (V,) or counts.shape != (V, keep) or (n >= 0 and int(win_offs[-1]) > V):
        raise ValueError("rows [V][keep], n_rows [V], counts [V][keep] and win_offsets[n] <= V")
    records, segments = np.zeros(V, dtype=capi.WINDOW_RECORD), np.zeros(V, dtype=capi.WINDOW_SEGMENT)
    n_segments = np.zeros(n, np.uint32)
    capi.check(lib.epik_amd_windows_paint_host(rows.ctypes.data, n_rows.ctypes.data, counts.ctypes.data, win_offs.ctypes.data, n,
                                               keep, group.ctypes.data, len(group), int(tau_q), records.ctypes.data,
                                               segments.ctypes.data, n_segments.ctypes.data))
    return records, segments, n_segments


def segment_span(seg, length: int, window: int, step: int):
    """[start, end) of a segment in its read: from the start of its first window to the end of its last."""
    first, last = int(seg["first_window"]), int(seg["first_window"]) + int(seg["num_windows"]) - 1
    return window_span(length, window, step, first)[0], window_span(length, window, step, last)[1]


def breakpoints(segments, length: int, window: int, step: int):
    """The breakpoints of one read from its segments (in order): for every two consecutive CALLED segments of different
    groups -- uncalled segments between them skipped -- (left call, right call, from, to), [from, to) running from the
    start of the left segment's last window to the end of the right segment's first window."""
    out, left = [], None
    for seg in segments:
        if int(seg["call"]) >= CALLED_BELOW:
            continue
        if left is not None and int(left["call"]) != int(seg["call"]):
            last = int(left["first_window"]) + int(left["num_windows"]) - 1
            out.append((int(left["call"]), int(seg["call"]), window_span(length, window, step, last)[0],
                        window_span(length, window, step, int(seg["first_window"]))[1]))
        left = seg
    return out


def call_name(call: int, group_paths) -> str:
    call = int(call)
    return capi.WINDOW_CLASSES[call] if call >= CALLED_BELOW else group_paths[call]


def _per_read(win_offs, n_segments, segments):
    win_offs = np.asarray(win_offs).astype(np.int64)
    for i in range(len(win_offs) - 1):
        yield i, segments[win_offs[i]:win_offs[i] + int(n_segments[i])]


def format_windows_tsv(names, lengths, win_offs, segments, n_segments, group_paths, window, step, tau_q, rank=1) -> str:
    """windows_<input>.tsv: per read, in order, one line per segment."""
    out = [f"# epik_amd windows v1\twindow={window}\tstep={step}\ttau_q={int(tau_q)}\tgroups={len(group_paths)}\trank={rank}"
           f"\trecords={len(names)}\n"]
    out += [f"# group\t{g}\t{path}\n" for g, path in enumerate(group_paths)]
    out.append("name\tsegment\tstart\tend\twindows\tcall\tsupport\n")
    for i, segs in _per_read(win_offs, n_segments, segments):
        for s, seg in enumerate(segs):
            start, end = segment_span(seg, int(lengths[i]), window, step)
            called = int(seg["call"]) < CALLED_BELOW
            support = "%.17g" % (float(int(seg["call_mass"])) / float(int(seg["total"]))) if called else "NA"
            out.append(f"{names[i]}\t{s}\t{start}\t{end}\t{int(seg['num_windows'])}\t{call_name(seg['call'], group_paths)}\t{support}\n")
    return "".join(out)


def format_breakpoints_tsv(names, lengths, win_offs, segments, n_segments, group_paths, window, step) -> str:
    """windows_breakpoints_<input>.tsv."""
    out = ["name\tleft\tright\tfrom\tto\n"]
    for i, segs in _per_read(win_offs, n_segments, segments):
        for left, right, lo, hi in breakpoints(segs, int(lengths[i]), window, step):
            out.append(f"{names[i]}\t{group_paths[left]}\t{group_paths[right]}\t{lo}\t{hi}\n")
    return "".join(out)


def format_windows_all_tsv(names, lengths, win_offs, records, rows, n_rows, strand, group_paths, window, step) -> str:
    """windows_all_<input>.tsv (--windows-per-window): one line per window."""
    out = ["name\twindow\tstart\tend\tstrand\tcall\tshare\tbest_edge_num\tbest_lwr\n"]
    win_offs = np.asarray(win_offs).astype(np.int64)
    for i in range(len(win_offs) - 1):
        for w in range(int(win_offs[i + 1] - win_offs[i])):
            v = win_offs[i] + w
            b, e = window_span(int(lengths[i]), window, step, w)
            rec = records[v]
            called = int(rec["call"]) < CALLED_BELOW
            share = "%.17g" % (float(rec["call_mass_q"]) / float(rec["total_q"])) if called else "NA"
            has = 0 < int(n_rows[v]) != capi.ROWS_COUNTS_TOO_NARROW
            edge, lwr = (str(int(rows[v, 0]["branch"])), "%.17g" % float(rows[v, 0]["lwr"])) if has else ("NA", "NA")
            out.append(f"{names[i]}\t{w}\t{b}\t{e}\t{'-' if strand is not None and strand[v] else '+'}\t"
                       f"{call_name(rec['call'], group_paths)}\t{share}\t{edge}\t{lwr}\n")
    return "".join(out)


def read_windows_tsv(text: str) -> dict:
    """What `format_windows_tsv` wrote: {"header": {key: int}, "groups": [taxopath], "segments": [(name, segment, start,
    end, windows, call, support or None)]}."""
    header, groups, segments = {}, [], []
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines or not lines[0].startswith("# epik_amd windows v1"):
        raise ValueError("not a windows file: the first line must begin with '# epik_amd windows v1'")
    for item in lines[0].split("\t")[1:]:
        key, _, value = item.partition("=")
        header[key] = int(value)
    at = 1
    while at < len(lines) and lines[at].startswith("# group\t"):
        _, g, path = lines[at].split("\t", 2)
        if int(g) != len(groups):
            raise ValueError(f"line {at + 1}: group {g} out of order")
        groups.append(path)
        at += 1
    if at >= len(lines) or lines[at] != "name\tsegment\tstart\tend\twindows\tcall\tsupport":
        raise ValueError(f"line {at + 1}: the column names are missing")
    for number, line in enumerate(lines[at + 1:], at + 2):
        f = line.split("\t")
        if len(f) != 7:
            raise ValueError(f"line {number}: 7 columns expected, not {len(f)}")
        segments.append((f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4]), f[5], None if f[6] == "NA" else float(f[6])))
    return {"header": header, "groups": groups, "segments": segments}
