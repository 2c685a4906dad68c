"""Top-k selection, the ratio filter and the team merge on the planted scenes of test_select_edges_cpu.py: every read of every
database against the CPU oracle through conftest.assert_rows_match -- row counts, branch order, float32 scores as uint32 bits
and k-mer counts equal bit for bit, the like-weight ratio within 1e-5.

* the one-wavefront kernel (candidate counts 1 .. 193 on both sides of the readlane ranking, the two broadcast rankings and the
  repeated selection; ties over the keep boundary, among all lane maxima and at tau; scores a unit apart, 2^8 .. 2^24 units
  apart and across binades; touched against keep; zero and tiny numerators, with k = 6 those whose quotient only the redone
  division rounds as IEEE does) in four layouts and three count widths, at
  keep = 1, 2, 7, 63 and 64, keep_factor 0.0, 0.01, 1.0 and the largest double, N = 600, 256, 63 and 3, k = 4 (exact
  quotients) and k = 5;
* a wave that places scene after scene (paired-fewblocks);
* the team kernels in eight layouts with M = slices * keep = 16, 18, 20, 32, 36, 64, 66, 72 (and 28, 56, 128 ...), the packed
  merges once more with a wave per read, slices of 17, 65 and 130 rows, and the touched-quad epilogue on 1 .. 257 quads.

That each scene reaches the seam it is named for is asserted in the CPU file, on the oracle and the restated bookkeeping
alone; the oracle's answers are computed once there and shared.
"""
import ctypes

import pytest

from conftest import assert_rows_match, select_kernel
from epik_amd import capi
from test_select_edges_cpu import (QUAD_N, TEAM_KEEPS, TEAM_LAYOUTS, TEAM_N, WAVE_CAP, all_runs, corrected_rows, database,
                                   dense_lanes, ks_of, merge_form, reference, select_model, settings)

pytestmark = pytest.mark.gpu

WIDE_COUNTS = {"u16": "0", "u32": "1", "u8": "2"}    # EPIK_AMD_WIDE_COUNTS
COUNT_CODE = {"u8": 0, "u16": 1, "u32": 2}           # epik_amd::CountBits
WAVE_LAYOUTS = ["paired", "packed", "compact", "paired-runs"]
WAVE_DATABASES = ("wave", "wave2", "runs", "stale", "div6", "n256", "n63", "n3")
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
    select_kernel(monkeypatch, layout)
    if counts is not None:
        monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", WIDE_COUNTS[counts])


def _place(placer_cls, oracle_lib, name, k, keep, factor, inspect=None, again=None):
    """One placement of a database's reads against the oracle.  inspect(pl): assertions on the handle after the launch.
    again(): called between a first and a second launch on the same handle, which is compared as well."""
    db, reads, (data, offs), scenes, n, slices = database(name, k)
    ref = reference(oracle_lib, name, k, keep, factor)
    with placer_cls.from_synth(db, keep_at_most=keep, keep_factor=factor) as pl:
        got = pl.place_packed(data, offs)
        if inspect is not None:
            inspect(pl)
        second = None
        if again is not None:
            again()
            second = pl.place_packed(data, offs)
    assert_rows_match(*got, *ref)
    if second is not None:
        assert_rows_match(*second, *ref)
    return len(reads)


@pytest.mark.parametrize("counts", ["u16", "u32", "u8"])
@pytest.mark.parametrize("layout", WAVE_LAYOUTS)
def test_wave_kernel_selection(placer_cls, oracle_lib, monkeypatch, layout, counts):
    """Every scene of the one-wavefront databases at every (keep, factor) of `settings`, k = 4 and 5.  The three count widths
    load a trip's rows differently; the run-coded layout keeps a list of one ascending run without its cells and, where every
    list of the database is one, counts per list."""
    _select(monkeypatch, layout, counts)
    placed = 0
    for name in WAVE_DATABASES:
        for k in ks_of(name):
            db = database(name, k)[0]
            want_lists = int(layout.endswith("-runs") and counts != "u8" and all_runs(db))

            def inspect(pl):
                lists = ctypes.c_uint32(7)
                assert pl._lib.epik_amd_placer_run_counts(pl._handle, COUNT_CODE[counts], ctypes.byref(lists)) == 0
                assert lists.value == want_lists, (name, k, lists.value)
                assert pl.last_path() == capi.PATH_WAVE and pl.partial_info()["slices"] == 1

            for keep, factor in settings(name):
                placed += _place(placer_cls, oracle_lib, name, k, keep, factor, inspect)
    assert placed > 900, placed


def test_a_wave_places_scene_after_scene(placer_cls, oracle_lib, monkeypatch):
    """Two workgroups on the device: a wave places a few dozen scenes one after the other, and a candidate list, a rank or a
    row that the previous read left behind would show in the next.  Both ends of the candidate counts lie side by side in the
    databases: 193 candidates, then 8; 206, then 5.  The "stale" database is made for this test: reads that leave 192 high
    candidates in the list, and behind them reads whose ranking reads one, two and three entries past their own."""
    _select(monkeypatch, "paired-fewblocks")

    def inspect(pl):
        assert pl.last_path() == capi.PATH_WAVE

    db, _, _, scenes, _, _ = database("wave", 4)
    sizes = [select_model(dense_lanes(rows), scores, sc.keep, WAVE_CAP)["n_cand"]
             for sc in scenes for rows, scores, _, _ in [corrected_rows(db, sc.read)]]
    assert max(sizes) > WAVE_CAP and min(sizes) == 0 and len(sizes) > 2 * 4 * 4   # (two workgroups of four waves: five scenes a wave)
    for name in ("wave", "wave2", "runs", "stale"):
        for k in (4, 5):
            for keep, factor in ((7, 0.01), (64, 0.01), (1, 0.01)):
                _place(placer_cls, oracle_lib, name, k, keep, factor, inspect)


@pytest.mark.parametrize("layout", sorted(TEAM_LAYOUTS))
def test_team_kernels_selection_and_merge(placer_cls, oracle_lib, monkeypatch, layout):
    """The slice epilogues and every form of the merge: keep chosen so that M = slices * keep lies on both sides of 16, 32 and
    64.  The packed merges (M <= 32) run once more with EPIK_AMD_MERGE_PACKED=0, a slot per lane."""
    _select(monkeypatch, layout)
    slices = TEAM_LAYOUTS[layout]
    name, n = f"team{slices}", TEAM_N[slices]
    forms = set()

    def inspect(pl):
        part = pl.partial_info()
        assert (part["slices"], part["slice_rows"]) == (slices, -(-n // slices)), part
        assert pl.last_path() == (capi.PATH_TEAM_ONE_KERNEL if layout.endswith("-classic") else capi.PATH_TEAM_STREAMED)
        build = pl.stream_build()
        if layout.endswith("-sparse"):
            assert build == {"wide": True, "sparse_quads": 256}, build
        elif layout.endswith("-dense"):
            assert build == {"wide": True, "sparse_quads": 0}, build
        elif not layout.endswith("-classic"):
            assert not build["wide"], build

    assert set(TEAM_KEEPS[slices]) < {keep for keep, _ in settings(name)}
    for k in (4, 5):
        for keep, factor in settings(name):
            form = merge_form(slices, keep)
            forms.add(form)
            monkeypatch.delenv("EPIK_AMD_MERGE_PACKED", raising=False)
            unpack = (lambda: monkeypatch.setenv("EPIK_AMD_MERGE_PACKED", "0")) if form.startswith("packed") else None
            _place(placer_cls, oracle_lib, name, k, keep, factor, inspect, again=unpack)
    monkeypatch.delenv("EPIK_AMD_MERGE_PACKED", raising=False)
    if slices == 4:     # k = 6, tiny numerators in slice 1: the quotients that only the redone division rounds as IEEE does
        assert database("div6team", 6)[4:] == (n, slices)
        for keep, factor in settings("div6team"):
            _place(placer_cls, oracle_lib, "div6team", 6, keep, factor, inspect)
    assert forms >= {2: {"packed16", "packed32", "loop"}, 4: {"packed16", "packed32", "lanes", "loop"},
                     8: {"packed32", "lanes", "loop"}}[slices], forms


@pytest.mark.parametrize("counts", ["u16", "u8"])
@pytest.mark.parametrize("layout", ["team2-sparse", "team2-dense", "team2"])
def test_touched_quad_epilogue(placer_cls, oracle_lib, monkeypatch, layout, counts):
    """Slices of 1 050 rows in which a read touches 1, 63, 64, 65, 128, 129, 192, 193, 256 and 257 quads, the best rows in the
    first and the last of them: one, two, three and four trips of the touched-quad epilogue with a whole or a partial last
    trip, and the dense epilogue behind 256 quads -- against the dense epilogue of the other two builds on the same reads."""
    _select(monkeypatch, layout, counts)

    def inspect(pl):
        part = pl.partial_info()
        assert (part["slices"], part["slice_rows"]) == (2, QUAD_N // 2), part
        assert pl.last_path() == capi.PATH_TEAM_STREAMED
        if layout != "team2":
            assert pl.stream_build() == {"wide": True, "sparse_quads": 256 if layout == "team2-sparse" else 0}

    for k in (4, 5):
        for keep, factor in ((7, 0.01), (64, 0.01), (7, 0.0)):
            _place(placer_cls, oracle_lib, "quads", k, keep, factor, inspect)
