"""Which ring the one-wavefront kernel takes for run-coded lists (epik_amd_placer_plan_run_counts, no device): counts
kept per list where every kept list is a run and the counts are 16 or 32 bits; the per-chunk count ring for a
database with lists of scattered branches, for 8-bit counts, for the filtered layout unless EPIK_AMD_RUN_COUNTS=lists,
and everywhere under EPIK_AMD_RUN_COUNTS=ring."""
import ctypes

import pytest

from epik_amd import capi, placer as eplacer, synth

U8, U16, U32 = 0, 1, 2


def _run_counts(db, counts, shard_index=0, shard_count=1):
    desc, keep = eplacer.make_desc(db.offsets, db.values, states=db.states, kmer_size=db.kmer_size,
                                   num_branches=db.num_branches, threshold=db.threshold,
                                   log_threshold=db.log_threshold, keys=getattr(db, "keys", None),
                                   holds_shard=getattr(db, "shard", None))
    out = ctypes.c_uint32(7)
    capi.check(capi.load().epik_amd_placer_plan_run_counts(ctypes.byref(desc), shard_index, shard_count, 288 << 30,
                                                           counts, ctypes.byref(out)))
    del keep
    return out.value


@pytest.fixture
def env(monkeypatch):
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUN_COUNTS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    return monkeypatch


@pytest.mark.parametrize("layout", ["paired", "packed"])
def test_all_run_database_takes_list_counts(env, layout):
    env.setenv("EPIK_AMD_LAYOUT", layout)
    db = synth.make_db(119, kmer_size=5, seed=8, p_present=0.5, lognormal=(2.5, 1.5))
    assert eplacer.plan(db).run_coded == 1
    assert [_run_counts(db, c) for c in (U8, U16, U32)] == [0, 1, 1]
    assert _run_counts(db, U16, shard_index=1, shard_count=3) == 1


def test_filtered_layout_takes_list_counts_only_when_asked(env):
    db = synth.make_db(39, states="amino", kmer_size=3, seed=10, p_present=0.1, lognormal=(1.0, 1.0))
    assert eplacer.plan(db).layout == 4 and eplacer.plan(db).run_coded == 1
    assert [_run_counts(db, c) for c in (U8, U16, U32)] == [0, 0, 0]
    env.setenv("EPIK_AMD_RUN_COUNTS", "lists")
    assert [_run_counts(db, c) for c in (U8, U16, U32)] == [0, 1, 1]
    env.setenv("EPIK_AMD_LAYOUT", "packed")
    env.delenv("EPIK_AMD_RUN_COUNTS")
    assert [_run_counts(db, c) for c in (U8, U16, U32)] == [0, 1, 1]


def test_scattered_database_keeps_the_ring(env):
    db = synth.make_db(119, kmer_size=5, seed=8, p_present=0.5, lognormal=(2.5, 1.5), scattered=True)
    assert eplacer.plan(db).run_coded == 1
    assert [_run_counts(db, c) for c in (U8, U16, U32)] == [0, 0, 0]


def test_ring_forced_and_no_run_coding(env):
    db = synth.make_db(119, kmer_size=5, seed=8, p_present=0.5, lognormal=(2.5, 1.5))
    env.setenv("EPIK_AMD_RUN_COUNTS", "ring")
    assert _run_counts(db, U16) == 0 and _run_counts(db, U32) == 0
    env.setenv("EPIK_AMD_RUN_COUNTS", "lists")
    assert _run_counts(db, U16) == 1
    env.setenv("EPIK_AMD_RUNS", "0")                      # explicit cells: no run ring at all
    assert eplacer.plan(db).run_coded == 0 and _run_counts(db, U16) == 0
    env.setenv("EPIK_AMD_RUNS", "1")
    env.setenv("EPIK_AMD_LAYOUT", "compact")
    assert _run_counts(db, U16) == 0
    env.delenv("EPIK_AMD_LAYOUT")
    env.setenv("EPIK_AMD_KERNEL", "team")                 # the sliced layout has no run coding
    assert _run_counts(db, U16) == 0


def test_arguments_are_checked(env):
    db = synth.make_db(119, kmer_size=5, seed=8)
    with pytest.raises(Exception):
        _run_counts(db, 3)
