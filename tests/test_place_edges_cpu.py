"""Placement at the branch counts where the placement kernels have their seams, on databases whose best rows are planted there.

Every GPU placement test compares the kept rows (at most keep_at_most a read) with the CPU oracle bit for bit.  Two things
about the inputs of those tests let a kernel be wrong without the comparison noticing:

* the branch counts.  Below N = 1 984 (the one-wavefront kernel) the suite placed reads at N = 3, 5, 15, 17, 59, 79, 119, 199,
  299, 301, 599, 999, 1 199, 1 303, 1 399, 1 999 and 200 only; every tree of synth.make_tree has odd N, and none has
  N = n_pad - 1 with n_pad = (N + 1 rounded up to 64) (db_image.cpp, decide_kernel).  The constants of the kernel step at
  the sizes in between: the dummy row directly behind the last branch (N = 63, 127, 255, 1 023), a block of 64 rows for the
  dummy row alone (N = 64, 128, 256, 1 024), the epilogue's trips of 256 rows with a masked last trip (place_device.hpp,
  correction_sweep and the candidate scan), materialize_counts' trips of 1 024 rows, the -1 of a run that ends on the last
  branch and lands on the dummy row exactly when N = n_pad - 1 (add_run_count), the 64 slack rows behind the score vector,
  and the slack | clamp choice and the 4 / 2 / 1-wave workgroups of db_layout.h, which change with n_pad and count width;
* where the best rows lie.  With synth.make_db the last branch is a kept row of two reads in a thousand and branch 0 of few
  more, so a kernel that dropped, shifted or miscounted the last row, the last quad of a trip or the first row of a slice
  changes no kept row, and its term of the score sum is far below the 1e-5 bar on the like-weight ratio.

`seam_db` plants the best rows: k = 5 nucleotide, one list per code, each one ascending run of branches that contains the
code's TARGET row, where the posting scores log10(0.3 + 0.7 u) against log10(threshold (1 + u)) everywhere else.
`wave_targets` and `team_targets` name the rows on either side of every seam.  This file asserts, on the oracle alone, what
keeps the GPU sweep of test_place_edges_gpu.py from passing vacuously, restates the LDS rule of db_layout.h that the GPU file
predicts the ring form with, and holds the oracle itself to arithmetic done by hand on one, two and three branches.
`reference` computes the oracle's answer once per (N, targets, keep, form) and shares it with the GPU file.
"""
import math
import os

import numpy as np
import pytest

from epik_amd import alphabet, synth
from epik_amd.synth import PKDB_VALUE, SynthDB

K = 5
CODES = 4 ** K
RUN_LENGTHS = (1, 2, 3, 5, 38, 63, 64, 65, 66, 129, 130, 257)
AMBIGUOUS = "ACGT" * 3 + "N" + "ACGGT" * 20 + "R" + "TTGCA" * 10   # test_ring_form_gpu.AMBIGUOUS (that module needs a GPU)

# ---- the cases of the GPU file --------------------------------------------------------------------------------------
WAVE_N = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025,
          1215, 1216, 1217, 1279, 1280, 1471, 1472, 1983)
KEEP_N = (63, 64, 65, 1023, 1024)                 # ... where keep = 1 and keep = 64 run beside keep = 7
KEEPS = ((7, 0.01),)
EDGE_KEEPS = ((1, 0.0), (64, 0.01))
TEAM_SLICES = {"team2": 2, "team4": 4, "team4x2": 8, "team8": 8, "team4-classic": 4, "team4-sparse": 4, "team4-dense": 4,
               "team4-block2": 4, "team4-smallpool": 4}
# slice_rows R = 15, 16, 17 and 31, 32 or 63, 64, 65: on both sides of team_rows_pad = (R + 1 rounded up to 16)
TEAM_SEAM_N = {2: (30, 32, 34, 126, 128, 130), 4: (60, 64, 68, 252, 256, 260), 8: (120, 128, 136)}
# a last slice of one row, an empty last slice, two empty slices
TEAM_LAST_N = {2: (), 4: (13, 9), 8: (17,)}
CHOSEN_N = (1984, 2047, 2048, 4200, 4201, 9999)  # create()'s own choice of kernel and slices
STRAND_N = (63, 64, 1023, 1024)
STRAND_CHOSEN_N = 2048


def n_pad_of(num_branches):
    """db_image.cpp, decide_kernel: the branches and the dummy row, to whole 64-row blocks."""
    return (int(num_branches) + 1 + 63) & ~63


# ---- db_layout.h, restated ------------------------------------------------------------------------------------------
LDS_PER_CU, LDS_GRANULE, WAVES_PER_CU = 160 * 1024, 1280, 20
WAVE_DESC_BYTES = (3 * 64 + 8) * 8      # (EPIK_AMD_TILES_PER_PASS * 64 + EPIK_AMD_RING) * 8
WAVE_SLACK_BYTES = 64 * 4
COUNT_CODE = {"u8": 0, "u16": 1, "u32": 2}   # epik_amd::CountBits


def wave_lds_bytes(n_pad, counts):
    return (n_pad * (4 + (1 << counts)) + WAVE_DESC_BYTES + 15) & ~15


def wave_kernel_geometry(n_pad, counts, extra=0):
    """(resident waves a CU, waves a workgroup): workgroups of 4, 2 or 1 waves, whichever keeps most (a tie: the larger)."""
    best, block_waves = 0, 0
    for wpb in (4, 2, 1):
        block = wpb * (wave_lds_bytes(n_pad, counts) + extra)
        if block > LDS_PER_CU:
            continue
        units = (block + LDS_GRANULE - 1) // LDS_GRANULE
        blocks = 128 // max(units, 1)
        if blocks * wpb > WAVES_PER_CU:
            blocks = WAVES_PER_CU // wpb
        if blocks * wpb > best:
            best, block_waves = blocks * wpb, wpb
    return best, block_waves


def wave_kernel_resident_waves(n_pad, counts, extra=0):
    return wave_kernel_geometry(n_pad, counts, extra)[0]


def wave_slack_is_free(n_pad, counts):
    return wave_kernel_resident_waves(n_pad, counts, WAVE_SLACK_BYTES) == wave_kernel_resident_waves(n_pad, counts)


def team_rows_pad(slice_rows):
    return (slice_rows + 1 + 15) & ~15


# ---- the planted database -------------------------------------------------------------------------------------------
def wave_targets(num_branches):
    n = int(num_branches)
    rows = (0, 3, 4, 63, 64, 255, 256, 511, 512, 767, 768, 1023, 1024, n - 65, n - 64, n - 5, n - 4, n - 2, n - 1)
    return tuple(sorted({r for r in rows if 0 <= r < n}))


def team_targets(num_branches, slices):
    """The first row of every slice and the row before it, with 0, N - 2 and N - 1; at most 24 rows, the seams of the first, the
    last non-empty and one middle slice always among them."""
    n, rows_per_slice = int(num_branches), -(-int(num_branches) // int(slices))
    seam = lambda s: {r for r in (s * rows_per_slice - 1, s * rows_per_slice) if 0 <= r < n}
    last = (n - 1) // rows_per_slice               # the last slice that holds a branch
    must = {r for r in (0, n - 2, n - 1) if 0 <= r < n} | seam(0) | seam(1) | seam(last) | seam(max(last // 2, 1))
    rest = sorted(set().union(*[seam(s) for s in range(int(slices))]) - must)
    room = max(24 - len(must), 0)
    if len(rest) > room:
        rest = [rest[i] for i in np.linspace(0, len(rest) - 1, room).round().astype(int)] if room else []
    return tuple(sorted(must | set(rest)))


def seam_db(num_branches, targets, seed, scattered=False):
    """One ascending run per code (built as test_ring_form_gpu._db builds its runs): code c belongs to target
    targets[c % len(targets)], the run's length is drawn from RUN_LENGTHS and clipped to N, and it lies at random so that it
    contains the target.  scattered: the same postings with every third non-target posting of the lists longer than 3
    dropped -- those lists are no runs any more and keep their cells in a run-coded image."""
    n = int(num_branches)
    rng = np.random.default_rng(seed)
    target = np.asarray(targets, dtype=np.int64)[np.arange(CODES) % len(targets)]
    lens = np.minimum(rng.choice(np.asarray(RUN_LENGTHS), size=CODES), n).astype(np.int64)
    lo, hi = np.maximum(0, target - lens + 1), np.minimum(target, n - lens)
    assert (lo <= hi).all()
    starts = lo + np.floor(rng.random(CODES) * (hi - lo + 1)).astype(np.int64)
    key = np.repeat(np.arange(CODES), lens)
    within = np.arange(key.size) - (np.cumsum(lens) - lens)[key]
    branch = starts[key] + within
    on_target = branch == target[key]
    assert int(on_target.sum()) == CODES
    threshold = alphabet.score_threshold(1.5, K, 4)
    u = rng.random(key.size)
    score = np.where(on_target, np.log10(0.3 + 0.7 * u), np.log10(float(threshold) * (1.0 + u)))
    keep = np.ones(key.size, dtype=bool)
    if scattered:
        other = ~on_target
        nth = np.cumsum(other) - 1                                  # index among all non-target postings ...
        first = np.concatenate([[0], np.cumsum(other)])[(np.cumsum(lens) - lens)]
        nth = nth - first[key]                                      # ... and among those of the posting's own list
        keep = ~(other & (nth % 3 == 2) & (lens[key] > 3))
    values = np.empty(int(keep.sum()), dtype=PKDB_VALUE)
    values["branch"] = branch[keep].astype(np.uint32)
    values["score"] = score[keep].astype(np.float32)
    offsets = np.zeros(CODES + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(key[keep], minlength=CODES))
    return SynthDB(states="nucl", kmer_size=K, omega=1.5, num_branches=n, offsets=offsets, values=values, threshold=threshold)


def lists_are_runs(db):
    """Per code: the list is one ascending run of branches (db_image.cpp, is_run; every list here is shorter than 65 536)."""
    offsets = db.offsets.astype(np.int64)
    br = db.values["branch"].astype(np.int64)
    breaks = np.ones(br.size, dtype=np.int64)
    breaks[1:] = np.diff(br) != 1
    breaks[offsets[:-1]] = 0                                        # a list's first posting continues nothing
    total = np.concatenate([[0], np.cumsum(breaks)])
    return total[offsets[1:]] == total[offsets[:-1]]


def edge_reads(seed, n_random=400):
    """Random reads of 5 .. 151 letters, one of 900, one with IUPAC codes, two that find no k-mer at all (their rows are the first
    keep_at_most branches with count 0 -- branches the tree does not have when N < keep_at_most), one shorter than k, one empty."""
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), size=int(m))) for m in rng.integers(K, 152, size=n_random)]
    reads += ["".join(rng.choice(list("ACGT"), size=900)), AMBIGUOUS, "NNNNNNNN", "-" * 12, "ACG", ""]
    return reads


def short_batch(reads):
    """The reads that 8-bit counts hold, and their indices in `reads`."""
    index = np.asarray([i for i, r in enumerate(reads) if len(r) - K + 1 <= 255])
    return [reads[i] for i in index], index


_CACHE = {}


def case_inputs(num_branches, targets, scattered=False):
    """(db, reads, packed reads) of a case, built once."""
    key = ("inputs", int(num_branches), tuple(targets), bool(scattered))
    if key not in _CACHE:
        # 400 random reads put every target of the one-wavefront sweep among the best rows of five reads and more; the team
        # cases (N = 136 with 17 targets: four reads) take 600
        reads = edge_reads(seed=int(num_branches) + 11, n_random=400 if tuple(targets) == wave_targets(num_branches) else 600)
        _CACHE[key] = (seam_db(num_branches, targets, seed=int(num_branches) + 5, scattered=scattered), reads,
                       synth.pack_reads(reads))
    return _CACHE[key]


def reference(oracle_lib, num_branches, targets, keep=7, factor=0.01, scattered=False, reverse=False):
    """The oracle's (rows, n_rows, counts) of a case, computed once and shared; the arrays are read-only.  reverse: of the
    reads' reverse complements (test_strand_gpu.oracle_strands)."""
    key = ("ref", int(num_branches), tuple(targets), int(keep), float(factor), bool(scattered), bool(reverse))
    if key not in _CACHE:
        db, reads, (data, offs) = case_inputs(num_branches, targets, scattered)
        if reverse:
            comp = str.maketrans("ACGTUacgtuRYKMBVDHrykmbvdhSWNswn", "TGCAAtgcaaYRMKVBHDyrmkvbhdSWNswn")
            data, offs = synth.pack_reads([r.translate(comp)[::-1] for r in reads])
        out = oracle_lib.Oracle.from_synth(db, keep_at_most=keep, keep_factor=factor).place(data, offs, num_threads=0)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def chosen_slices(num_branches):
    """Slices of the branch range that create() takes by itself for a tree of N branches (epik_amd_placer_plan_sizes: no device)."""
    from epik_amd import placer
    key = ("slices", int(num_branches))
    if key not in _CACHE:
        saved = {v: os.environ.pop(v, None) for v in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS")}
        try:
            p = placer.plan_sizes(states="nucl", kmer_size=K, num_branches=int(num_branches), bins=[(64, CODES, CODES)])
        finally:
            os.environ.update({k: v for k, v in saved.items() if v is not None})
        assert p.team_waves * p.team_passes >= 2, "a tree of 1 984 branches and more takes the team kernels"
        assert p.slice_rows == -(-int(num_branches) // (p.team_waves * p.team_passes))
        _CACHE[key] = int(p.team_waves * p.team_passes)
    return _CACHE[key]


def team_cases():
    """(N, slices) of every forced team case of the GPU file."""
    return sorted({(n, s) for s in TEAM_SEAM_N for n in TEAM_SEAM_N[s] + TEAM_LAST_N[s]})


def all_cases():
    """(N, targets) of every database the GPU file places reads on."""
    cases = [(n, wave_targets(n)) for n in WAVE_N]
    cases += [(n, team_targets(n, s)) for n, s in team_cases()]
    cases += [(n, team_targets(n, chosen_slices(n))) for n in CHOSEN_N]
    cases += [(STRAND_CHOSEN_N, team_targets(STRAND_CHOSEN_N, chosen_slices(STRAND_CHOSEN_N)))]
    return sorted(set(cases))


# ---- (1) the conditions that keep the GPU sweep from passing vacuously ----------------------------------------------
def test_targets_name_the_seams():
    assert wave_targets(1) == (0,) and wave_targets(2) == (0, 1) and wave_targets(5) == (0, 1, 3, 4)
    assert wave_targets(64) == (0, 3, 4, 59, 60, 62, 63) and wave_targets(63)[-3:] == (59, 61, 62)
    assert {958, 959, 1018, 1019, 1021, 1022}.issubset(wave_targets(1023)) and 1023 not in wave_targets(1023)
    assert {1023, 959, 960, 1019, 1020, 1022}.issubset(wave_targets(1024))
    assert len(wave_targets(1983)) == 19
    assert team_targets(64, 4) == (0, 15, 16, 31, 32, 47, 48, 62, 63)
    assert team_targets(13, 4) == (0, 3, 4, 7, 8, 11, 12)               # R = 4: the last slice holds branch 12 alone
    assert team_targets(9, 4) == (0, 2, 3, 5, 6, 7, 8)                  # R = 3: slice 3 is empty
    assert team_targets(17, 8) == (0, 2, 3, 5, 6, 8, 9, 11, 12, 14, 15, 16)
    many = team_targets(9999, 40)                                       # R = 250: thinned, the named seams kept
    assert len(many) == 24 and {0, 249, 250, 9749, 9750, 9997, 9998, 4749, 4750}.issubset(many)
    for n, s in team_cases():
        assert {0, n - 1}.issubset(team_targets(n, s))
    # on both sides of team_rows_pad's step: R = 15 and 31 fill their padded rows with the dummy row, 16 and 32 open another 16
    assert [team_rows_pad(r) for r in (15, 16, 17, 31, 32, 63, 64, 65)] == [16, 32, 32, 32, 48, 64, 80, 80]
    assert sorted({-(-n // s) for s in TEAM_SEAM_N for n in TEAM_SEAM_N[s]}) == [15, 16, 17, 63, 64, 65]


def test_scattered_lists_take_the_explicit_arm():
    for n in (4, 5, 63, 1024):
        base, form = seam_db(n, wave_targets(n), 3), seam_db(n, wave_targets(n), 3, scattered=True)
        assert lists_are_runs(base).all()
        lens = np.diff(base.offsets.astype(np.int64))
        runs = lists_are_runs(form)
        assert (runs[lens <= 3]).all() and np.array_equal(np.diff(form.offsets.astype(np.int64))[lens <= 3], lens[lens <= 3])
        if n >= 5:
            assert not runs[lens > 3].any() and (lens > 3).sum() > 300
        # the same postings: what is left of a list is a subset of the run, the target's posting with its score among it
        a = {(int(c), int(b)): float(s) for c, b, s in zip(np.repeat(np.arange(CODES), lens), base.values["branch"], base.values["score"])}
        lens2 = np.diff(form.offsets.astype(np.int64))
        b = {(int(c), int(r)): float(s) for c, r, s in zip(np.repeat(np.arange(CODES), lens2), form.values["branch"], form.values["score"])}
        assert set(b) <= set(a) and all(a[key] == b[key] for key in b)
        best = {c: max((s, r) for (cc, r), s in b.items() if cc == c)[1] for c in range(0, CODES, 37)}
        assert all(best[c] == wave_targets(n)[c % len(wave_targets(n))] for c in best)


def test_every_target_is_a_best_row_and_the_edges_hold_lists(oracle_lib):
    worst = {"best": (10 ** 9, 0), "kept": (10 ** 9, 0), "share": (2.0, 0), "ends": (10 ** 9, 0), "starts": (10 ** 9, 0)}
    for n, targets in all_cases():
        for scattered in (False, True):
            db, reads, _ = case_inputs(n, targets, scattered)
            rows, n_rows, counts = reference(oracle_lib, n, targets, scattered=scattered)
            valid = np.arange(rows.shape[1])[None, :] < n_rows[:, None]
            found = valid & (counts > 0)
            best = rows["branch"][:, 0][found[:, 0]]
            kept = rows["branch"][found]
            for t in targets:
                b, k_ = int((best == t).sum()), int((kept == t).sum())
                assert b >= 5 and k_ >= 50, f"N = {n}, target {t}: best row of {b} reads, kept row of {k_}"
                worst["best"], worst["kept"] = min(worst["best"], (b, n)), min(worst["kept"], (k_, n))
            worst["share"] = min(worst["share"], (float(np.isin(kept, targets).mean()), n))
            offsets = db.offsets.astype(np.int64)
            ends = int((db.values["branch"][offsets[1:] - 1] == n - 1).sum())
            starts = int((db.values["branch"][offsets[:-1]] == 0).sum())
            if n >= 64:
                assert ends >= 20 and starts >= 20, f"N = {n}: {ends} lists end on the last branch, {starts} start on branch 0"
                worst["ends"], worst["starts"] = min(worst["ends"], (ends, n)), min(worst["starts"], (starts, n))
            # a read that found no k-mer keeps rows of count 0 (the first keep branches), and some read keeps fewer than keep
            assert (valid & (counts == 0)).any(), n
            assert ((n_rows > 0) & (n_rows < rows.shape[1])).any(), n
            if n < rows.shape[1]:   # fewer branches than rows to keep: the rows of a read without k-mers name branches past the tree
                assert int(rows["branch"][valid].max()) == rows.shape[1] - 1 >= n
    print("worst (value, N):", worst)


def test_other_keeps_still_reach_the_targets(oracle_lib):
    """keep = 1 (the best row alone) and keep = 64 (N = 63 | 64 | 65: every branch of the tree | all but one | two a row)."""
    for n in KEEP_N:
        targets = wave_targets(n)
        for keep, factor in EDGE_KEEPS:
            rows, n_rows, counts = reference(oracle_lib, n, targets, keep=keep, factor=factor)
            valid = (np.arange(keep)[None, :] < n_rows[:, None]) & (counts > 0)
            kept = rows["branch"][valid]
            assert all(int((kept == t).sum()) >= 5 for t in targets), (n, keep)
            assert int(n_rows.max()) == keep       # (the reads without a k-mer, if no other)


# ---- (2) the LDS rule of db_layout.h ---------------------------------------------------------------------------------
def test_lds_rule_restated():
    # the four values db_layout.h asserts statically
    assert wave_kernel_resident_waves(1024, 1, WAVE_SLACK_BYTES) == 20 and wave_slack_is_free(1024, 2)
    assert wave_kernel_resident_waves(1216, 1) == 18 and wave_kernel_resident_waves(1216, 1, WAVE_SLACK_BYTES) == 16
    assert wave_kernel_resident_waves(1216, 2) == 14 and wave_kernel_resident_waves(1216, 2, WAVE_SLACK_BYTES) == 12
    assert wave_lds_bytes(1024, 1) == 7744                            # "4 x (7 744 + 256) B = the 25 granules"
    # among the sizes of the sweep the clamp is expected at n_pad 1 216 (both widths), 1 472 and 1 536 (32-bit counts) ...
    pads = sorted({n_pad_of(n) for n in WAVE_N})
    assert pads == [64, 128, 192, 256, 320, 512, 576, 768, 832, 1024, 1088, 1216, 1280, 1344, 1472, 1536, 1984]
    clamp = {(p, c) for p in pads for c in ("u16", "u32") if not wave_slack_is_free(p, COUNT_CODE[c])}
    assert clamp == {(1216, "u16"), (1216, "u32"), (1472, "u32"), (1536, "u32")}
    # ... and by the same rule at 1 408 and 2 048 with 16-bit counts, sizes no swept N pads to
    assert not wave_slack_is_free(1408, 1) and not wave_slack_is_free(2048, 1)
    # workgroups of four and of two waves both occur, and of one at N = 1 472 with 32-bit counts: 11 waves a CU
    assert wave_kernel_geometry(n_pad_of(1472), 2) == (11, 1)
    for c in (0, 1, 2):
        assert {wave_kernel_geometry(p, c)[1] for p in pads} >= {4, 2}
    # N = n_pad - 1 | n_pad: the dummy row directly behind the last branch | in a block of its own
    assert [n_pad_of(n) for n in (63, 64, 1023, 1024, 1215, 1216, 1983)] == [64, 128, 1024, 1088, 1216, 1280, 1984]
    # a last chunk of one posting at row N - 1 has its 64 lanes at rows N - 1 .. N + 62 = n_pad + 61 when N = n_pad - 1
    assert (1023 - 1) + 63 == n_pad_of(1023) + 61 and n_pad_of(1023) + 64 - 1 == n_pad_of(1023) + 63


# ---- (3) the oracle on one, two and three branches, against arithmetic by hand -------------------------------------
def _by_hand(db, read, keep, factor):
    """A read of plain letters on a tree of a few branches: every k-mer has one list; a row's score is the float32 sum of its
    postings in the read's order, plus the threshold's logarithm for every k-mer that missed it, over k."""
    f32 = np.float32
    n_kmers = len(read) - K + 1
    if n_kmers < 1:
        return []
    total, count = [f32(0)] * db.num_branches, [0] * db.num_branches
    for p in range(n_kmers):
        code = int("".join(str("ACGT".index(ch)) for ch in read[p:p + K]), 4)
        for v in db.values[int(db.offsets[code]):int(db.offsets[code + 1])]:
            total[int(v["branch"])] = f32(total[int(v["branch"])] + v["score"])
            count[int(v["branch"])] += 1
    log_thr = f32(db.log_threshold)
    rows = [(b, f32(f32(total[b] + f32(f32(n_kmers - count[b]) * log_thr)) / f32(K)), count[b])
            for b in range(db.num_branches) if count[b]]
    unplaced = float(f32(f32(db.num_branches) - f32(len(rows)))) * math.pow(10.0, float(f32(f32(f32(n_kmers) * log_thr) / f32(K))))
    score_sum = unplaced + sum(math.pow(10.0, float(s)) for _, s, _ in rows)
    rows = sorted(rows, key=lambda r: (-float(r[1]), r[0]))[:keep]
    out = [(b, s, math.pow(10.0, float(s)) / score_sum, c) for b, s, c in rows]
    return [r for r in out if r[2] >= out[0][2] * factor]


@pytest.mark.parametrize("num_branches", [1, 2, 3])
def test_oracle_on_one_two_and_three_branches(oracle_lib, num_branches):
    targets = wave_targets(num_branches)
    for scattered in (False, True):
        db, reads, _ = case_inputs(num_branches, targets, scattered)
        for keep, factor in ((7, 0.01), (1, 0.0), (2, 0.5)):
            rows, n_rows, counts = reference(oracle_lib, num_branches, targets, keep=keep, factor=factor, scattered=scattered)
            checked = 0
            for i, read in enumerate(reads):
                if set(read) - set("ACGT"):
                    continue
                want = _by_hand(db, read, keep, factor)
                assert int(n_rows[i]) == len(want), (i, read)
                for j, (b, s, lwr, c) in enumerate(want):
                    assert int(rows[i, j]["branch"]) == b and int(counts[i, j]) == c
                    assert np.float32(rows[i, j]["score"]).view(np.uint32) == np.float32(s).view(np.uint32)
                    assert abs(float(rows[i, j]["lwr"]) - lwr) <= 1e-12 * lwr
                checked += 1
            assert checked >= 400
            # the two reads without a k-mer: the first `keep` branches at the threshold score, count 0 -- whatever the tree holds
            for read in ("NNNNNNNN", "-" * 12):
                i = reads.index(read)
                thr = np.float32(np.float32(np.float32(len(read) - K + 1) * np.float32(db.log_threshold)) / np.float32(K))
                assert int(n_rows[i]) == keep and list(rows[i]["branch"]) == list(range(keep)) and not counts[i].any()
                assert (rows[i]["score"].view(np.uint32) == thr.view(np.uint32)).all()
