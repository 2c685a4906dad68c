"""The placement kernels at their branch-count seams, on the planted databases of test_place_edges_cpu.py: every read of every
case against the CPU oracle through conftest.assert_rows_match -- row counts, branch order, float32 scores as uint32 bits and
k-mer counts equal bit for bit, the like-weight ratio within 1e-5.

* the one-wavefront kernel at 32 branch counts from 1 to 1 983 (N = n_pad - 1 and n_pad on either side of every 64-row block
  that matters, the 256-row trips of the epilogue, the 1 024-row trips of materialize_counts), in eight layouts and three
  count widths, on databases of runs and of explicit-cell lists; keep = 7 everywhere, keep = 1 and 64 at 63, 64, 65, 1 023
  and 1 024.  The run-coded layouts also report which kernel and ring form they took, held to the restated rule of
  db_layout.h: list counts with slack rows, list counts with the clamp and the run ring are each seen in every width;
* the team kernels with slices of 15, 16, 17 and 31, 32 (63, 64, 65) rows, last slices of one row and of none, and the
  geometries create() picks at N = 1 984 .. 9 999, with best rows on the first and the last row of every slice;
* both strands at N = 63, 64, 1 023, 1 024 and 2 048 (strand_place.hip instantiates the same epilogue).

What makes these inputs reach the seams -- every target a best row of five reads and more, lists that end on N - 1 and start on
0, rows of count 0 -- is asserted in the CPU file on the oracle alone; the oracle's answers are computed once there and shared.
"""
import ctypes

import numpy as np
import pytest

from conftest import assert_rows_match, select_kernel
from epik_amd import capi, synth
from test_place_edges_cpu import (CHOSEN_N, COUNT_CODE, EDGE_KEEPS, KEEP_N, KEEPS, STRAND_CHOSEN_N, STRAND_N, TEAM_LAST_N,
                                  TEAM_SEAM_N, TEAM_SLICES, WAVE_N, WAVE_SLACK_BYTES, case_inputs, chosen_slices,
                                  lists_are_runs, n_pad_of, reference, short_batch, team_targets, wave_kernel_geometry,
                                  wave_lds_bytes, wave_slack_is_free, wave_targets)
from test_strand_gpu import both_rule

pytestmark = pytest.mark.gpu

NEAR, SLACK = 1, 2                                   # EPIK_AMD_RING_NEAR, EPIK_AMD_RING_SLACK
WIDE_COUNTS = {"u16": "0", "u32": "1", "u8": "2"}    # EPIK_AMD_WIDE_COUNTS
WAVE_LAYOUTS = ["paired", "packed", "compact", "filtered", "packed-runs", "paired-runs", "paired-runs-far", "paired-fewblocks"]
ENV = ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_RING_FORM", "EPIK_AMD_WIDE_COUNTS", "EPIK_AMD_TEAM_TABLE", "EPIK_AMD_HOST_CHUNKS",
       "EPIK_AMD_MERGE_PACKED", "EPIK_AMD_SPARSE_DESC")


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _select(monkeypatch, layout, counts=None):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    if layout is None:   # what create() chooses
        select_kernel(monkeypatch, "paired")
        for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT"):
            monkeypatch.delenv(var, raising=False)
    elif layout.endswith("-far"):
        select_kernel(monkeypatch, layout[:-len("-far")])
        monkeypatch.setenv("EPIK_AMD_RING_FORM", "far")
    else:
        select_kernel(monkeypatch, layout)
    if counts is not None:
        monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", WIDE_COUNTS[counts])


def _subset(ref, index):
    return tuple(a[index] for a in ref)


@pytest.mark.parametrize("counts", ["u16", "u32", "u8"])
@pytest.mark.parametrize("layout", WAVE_LAYOUTS)
def test_wave_kernel_at_the_seams(placer_cls, oracle_lib, monkeypatch, layout, counts):
    """Every N of the sweep in both database forms, keep = 7 (and 1 and 64 at KEEP_N).  On the MI355X the handle takes the
    workgroup of the restated rule at every case: four waves, two (N = 1 024, 1 025, 1 215 ... with 16-bit counts) and ONE at
    N = 1 472 with 32-bit counts -- 11 waves a CU, as db_layout.h's rule gives -- and at N = 1 983 with 16- and 32-bit counts."""
    _select(monkeypatch, layout, counts)
    run_coded, far = "-runs" in layout, layout.endswith("-far")
    width = COUNT_CODE[counts]
    taken, block_waves, refused, cases, at_1472 = set(), set(), [], 0, None
    for n in WAVE_N:
        targets, n_pad = wave_targets(n), n_pad_of(n)
        for scattered in (False, True):
            db, reads, (data, offs) = case_inputs(n, targets, scattered)
            # 8-bit counts hold 255 k-mers: a longer read in the batch widens the launch, so the batch goes without it
            index = short_batch(reads)[1] if counts == "u8" else np.arange(len(reads))
            if counts == "u8":
                data, offs = synth.pack_reads([reads[i] for i in index])
            for keep, factor in KEEPS + (EDGE_KEEPS if n in KEEP_N else ()):
                cases += 1
                ref = _subset(reference(oracle_lib, n, targets, keep=keep, factor=factor, scattered=scattered), index)
                try:
                    pl = placer_cls.from_synth(db, keep_at_most=keep, keep_factor=factor)
                except capi.EpikAmdError as e:   # a layout without a kernel for this case: recorded, at most one case in ten
                    refused.append((n, scattered, keep, str(e)))
                    continue
                with pl:
                    assert pl.partial_info()["slices"] == 1
                    got = pl.place_packed(data, offs)
                    info = pl.launch_info()
                    lists, form = ctypes.c_uint32(7), ctypes.c_uint32(7)
                    assert pl._lib.epik_amd_placer_run_counts(pl._handle, width, ctypes.byref(lists)) == 0
                    assert pl._lib.epik_amd_placer_ring_form(pl._handle, width, ctypes.byref(form)) == 0
                    assert pl.last_path() == capi.PATH_WAVE
                worst = assert_rows_match(*got, *ref)
                assert worst <= 1e-5
                # which kernel and ring form: list counts where every list is a run and the counts are not 8 bits wide, the 64
                # slack rows where the restated rule of db_layout.h says they cost no resident wave
                want_lists = run_coded and counts != "u8" and bool(lists_are_runs(db).all())
                want_form = 0 if far or not run_coded else NEAR | (SLACK if want_lists and wave_slack_is_free(n_pad, width) else 0)
                assert (lists.value, form.value) == (int(want_lists), want_form), (n, scattered, lists.value, form.value)
                if run_coded:
                    taken.add("run ring" if not want_lists else "lists, far" if far else "lists, slack" if want_form & SLACK else "lists, clamp")
                # the launch took the width asked for: a wave's LDS is that of the rule (and the slack rows' 256 bytes)
                slack = WAVE_SLACK_BYTES if form.value & SLACK else 0
                assert info["lds_bytes_per_block"] == info["waves_per_block"] * (wave_lds_bytes(n_pad, width) + slack), (n, info)
                block_waves.add(info["waves_per_block"])
                # ... in the workgroup of the rule: four waves, two, or one (N = 1 472 with 32-bit counts: 11 waves a CU)
                assert info["waves_per_block"] == wave_kernel_geometry(n_pad, width, slack)[1], (n, info)
                if n == 1472:
                    at_1472 = (info["waves_per_block"], wave_kernel_geometry(n_pad, width, slack))
    print(f"{layout} {counts}: {cases} placements, {len(refused)} refused {refused[:3]}, forms {sorted(taken)}, waves a workgroup "
          f"{sorted(block_waves)}; N = 1 472: the handle takes {at_1472[0]}, the rule (waves a CU, waves a workgroup) {at_1472[1]}")
    assert len(refused) * 10 <= cases, refused
    assert {4, 2} <= block_waves, block_waves
    if run_coded:
        want = {"run ring"} if counts == "u8" else {"run ring", "lists, far"} if far else {"run ring", "lists, slack", "lists, clamp"}
        assert taken == want, (taken, want)


def _place_both_widths(pl, reads, data, offs):
    """The whole batch (its 900-letter read takes 16-bit counts) and the batch without it (8-bit counts where the kernel exists)."""
    short, index = short_batch(reads)
    return pl.place_packed(data, offs), pl.place_packed(*synth.pack_reads(short)), index


def _team_case(placer_cls, oracle_lib, n, slices):
    seen = set()
    targets = team_targets(n, slices)
    for scattered in (False, True):
        db, reads, (data, offs) = case_inputs(n, targets, scattered)
        ref = reference(oracle_lib, n, targets, scattered=scattered)
        with placer_cls.from_synth(db) as pl:
            part = pl.partial_info()
            assert (part["slices"], part["slice_rows"]) == (slices, -(-n // slices)), (n, part)
            got, got_short, index = _place_both_widths(pl, reads, data, offs)
            assert pl.last_path() != capi.PATH_WAVE
            seen.add(pl.last_path())
        assert_rows_match(*got, *ref)
        assert_rows_match(*got_short, *_subset(ref, index))
    return seen


@pytest.mark.parametrize("layout", sorted(TEAM_SLICES))
def test_team_kernels_at_the_slice_seams(placer_cls, oracle_lib, monkeypatch, layout):
    """Slices of R = 15, 16, 17 and 31, 32 (two and four slices: 63, 64, 65) rows, on both sides of team_rows_pad; then a last
    slice of one row (N = 13, four slices), an empty one (N = 9) and two empty ones (N = 17, eight slices)."""
    _select(monkeypatch, layout)
    slices = TEAM_SLICES[layout]
    paths = set()
    for n in TEAM_SEAM_N[slices] + TEAM_LAST_N[slices]:
        paths |= _team_case(placer_cls, oracle_lib, n, slices)
    assert paths == ({capi.PATH_TEAM_ONE_KERNEL} if layout.endswith("-classic") else {capi.PATH_TEAM_STREAMED}), paths


@pytest.mark.parametrize("num_branches", CHOSEN_N)
def test_the_geometry_create_chooses(placer_cls, oracle_lib, monkeypatch, num_branches):
    """No kernel and no layout forced: the team kernels from N = 1 984 on, two slices a pass up to 4 200 branches and four
    beyond, with the best rows on the seams of the slices the handle reports."""
    _select(monkeypatch, None)
    slices = chosen_slices(num_branches)
    assert slices % (2 if num_branches <= 4200 else 4) == 0
    _team_case(placer_cls, oracle_lib, num_branches, slices)


@pytest.mark.parametrize("layout", ["paired-runs", "packed", None])
def test_both_strands_at_the_seams(placer_cls, oracle_lib, monkeypatch, layout):
    """place_strands(mode="both") against the rule of test_strand_gpu on two oracle runs."""
    _select(monkeypatch, layout)
    for n in STRAND_N if layout else (STRAND_CHOSEN_N,):
        targets = wave_targets(n) if layout else team_targets(n, chosen_slices(n))
        db, reads, (data, offs) = case_inputs(n, targets)
        fwd, rev = reference(oracle_lib, n, targets), reference(oracle_lib, n, targets, reverse=True)
        want, want_strand = both_rule(fwd, rev)
        with placer_cls.from_synth(db) as pl:
            rows, n_rows, counts, strand = pl.place_strands(data, offs, "both")
            assert (pl.last_path() == capi.PATH_WAVE) == (layout is not None)
        assert_rows_match(rows, n_rows, counts, *want)
        assert np.array_equal(strand, want_strand)
        assert 50 < int(strand.sum()) < len(reads) - 50
