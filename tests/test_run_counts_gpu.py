"""The one-wavefront kernel with counts kept per list (place_device.hpp, RunListLayout): on a run-coded image whose
lists are all runs, with 16- or 32-bit counts, each list adds to its run's counts once and the posting ring carries
scores only.  Checked bit for bit against the CPU oracle, and against the per-chunk count ring
(EPIK_AMD_RUN_COUNTS=ring) for identical output: rows, scores as uint32 bits, LWR, k-mer counts."""
import numpy as np
import pytest

from conftest import assert_rows_match
from epik_amd import synth
from epik_amd.synth import PKDB_VALUE, SynthDB

pytestmark = pytest.mark.gpu

COUNTS = {"u16": "0", "u32": "1", "u8": "2"}  # EPIK_AMD_WIDE_COUNTS


def _run_db(num_branches, kmer_size=5, seed=3, lengths=(1, 2, 63, 64, 65, 128, 129, 200, 256)):
    """Every code present, each list one run: lengths drawn from `lengths` (capped at the tree), every fifth list
    ending at branch N - 1, and a few lists of the whole tree."""
    rng = np.random.default_rng(seed)
    num_keys = 4 ** kmer_size
    lens = np.minimum(rng.choice(np.asarray(lengths), size=num_keys), num_branches).astype(np.int64)
    lens[rng.choice(num_keys, size=8, replace=False)] = num_branches
    starts = (rng.random(num_keys) * (num_branches - lens + 1)).astype(np.int64)
    starts[::5] = num_branches - lens[::5]
    offsets = np.zeros(num_keys + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    values = np.empty(int(offsets[-1]), dtype=PKDB_VALUE)
    key = np.repeat(np.arange(num_keys), lens)
    within = np.arange(values.size) - (np.cumsum(lens) - lens)[key]
    values["branch"] = (starts[key] + within).astype(np.uint32)
    threshold = synth.alphabet.score_threshold(1.5, kmer_size, 4)
    values["score"] = np.log10(threshold + rng.random(values.size) * (1.0 - threshold)).astype(np.float32)
    return SynthDB(states="nucl", kmer_size=kmer_size, omega=1.5, num_branches=num_branches, offsets=offsets,
                   values=values, threshold=threshold)


def _reads(seed=5):
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(5, 260, size=300)]
    reads += ["".join(rng.choice(list("ACGT"), size=900)),       # many passes, rounds of more than 192 chunks
              "".join(rng.choice(list("ACGT"), size=3000)),
              "ACGTA" * 60,                                         # the same k-mers over and over
              "ACGT" * 3 + "N" + "ACGGT" * 20 + "R" + "TTGCA" * 10,  # IUPAC ambiguity
              "NNNNNNNN", "ACG", ""]
    reads += ["".join(rng.choice(list("ACGTNRY"), p=[.24, .24, .24, .24, .02, .01, .01], size=150)) for _ in range(40)]
    return synth.pack_reads(reads)


def _setup(monkeypatch, layout, counts, ring=False, blocks=True):
    for var in ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    monkeypatch.setenv("EPIK_AMD_LAYOUT", layout)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", COUNTS[counts])
    if blocks:
        monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", "2")  # a wave places several reads one after another
    if ring:
        monkeypatch.setenv("EPIK_AMD_RUN_COUNTS", "ring")


def _lists(pl, counts):
    import ctypes
    out = ctypes.c_uint32(7)
    assert pl._lib.epik_amd_placer_run_counts(pl._handle, {"u8": 0, "u16": 1, "u32": 2}[counts], ctypes.byref(out)) == 0
    return out.value


@pytest.mark.parametrize("counts", ["u16", "u32"])
@pytest.mark.parametrize("layout", ["paired", "packed"])
@pytest.mark.parametrize("num_branches", [60, 300, 999, 1500])
def test_list_counts_equal_the_oracle_and_the_ring(gpu_available, oracle_lib, monkeypatch, counts, layout, num_branches):
    from epik_amd.placer import Placer
    assert gpu_available
    db = _run_db(num_branches, seed=num_branches)
    data, offs = _reads(seed=num_branches + 1)
    ref = oracle_lib.Oracle.from_synth(db, keep_at_most=7).place(data, offs, num_threads=0)
    _setup(monkeypatch, layout, counts)
    with Placer.from_synth(db, keep_at_most=7) as pl:
        assert _lists(pl, counts) == 1
        got = pl.place_packed(data, offs)
    assert_rows_match(*got, *ref)
    _setup(monkeypatch, layout, counts, ring=True)
    with Placer.from_synth(db, keep_at_most=7) as pl:
        assert _lists(pl, counts) == 0
        old = pl.place_packed(data, offs)
    for a, b in zip(got, old):
        assert a.tobytes() == b.tobytes()


def test_u8_counts_keep_the_ring(gpu_available, oracle_lib, monkeypatch):
    from epik_amd.placer import Placer
    db = _run_db(300)
    data, offs = synth.make_reads(300, 150, seed=9)
    _setup(monkeypatch, "paired", "u8")
    with Placer.from_synth(db) as pl:
        assert _lists(pl, "u8") == 0 and _lists(pl, "u16") == 1
        got = pl.place_packed(data, offs)
    assert_rows_match(*got, *oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0))


@pytest.mark.parametrize("counts", ["u16", "u32"])
def test_synthetic_and_clade_databases(gpu_available, oracle_lib, monkeypatch, counts):
    from epik_amd.placer import Placer
    tree = synth.make_tree(500, seed=11)
    db = synth.make_db(tree.num_nodes, kmer_size=8, seed=12, p_present=0.6)
    cdb, refs, _ = synth.make_clade_db(999, kmer_size=8, n_refs=60, ref_length=600)
    cases = [(db, synth.make_reads(2000, 150, seed=13)), (cdb, synth.make_clade_reads(refs, 1000, 150, seed=14))]
    for d, (data, offs) in cases:
        ref = oracle_lib.Oracle.from_synth(d).place(data, offs, num_threads=0)
        _setup(monkeypatch, "paired", counts, blocks=False)
        with Placer.from_synth(d) as pl:
            lists = _lists(pl, counts)
            got = pl.place_packed(data, offs)
        assert_rows_match(*got, *ref)
        _setup(monkeypatch, "paired", counts, ring=True, blocks=False)
        with Placer.from_synth(d) as pl:
            old = pl.place_packed(data, offs)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, old))
        if d is db:
            assert lists == 1  # make_db's lists are all runs


def test_strands_and_frames_match_the_ring(gpu_available, monkeypatch):
    from epik_amd.placer import Placer
    db = _run_db(300, seed=21)
    data, offs = _reads(seed=22)
    amino = synth.make_db(200, states="amino", kmer_size=3, seed=23, p_present=0.5)
    out = {}
    for ring in (False, True):
        _setup(monkeypatch, "paired", "u16", ring=ring)
        with Placer.from_synth(db) as pl:
            assert _lists(pl, "u16") == (0 if ring else 1)
            out[ring, "strands"] = pl.place_strands(data, offs, "both")
        _setup(monkeypatch, "filtered", "u16", ring=ring)
        if not ring:  # (the filtered layout takes list counts only when asked: db_image.hpp run_counts_apply)
            monkeypatch.setenv("EPIK_AMD_RUN_COUNTS", "lists")
        with Placer.from_synth(amino) as pl:
            assert _lists(pl, "u16") == (0 if ring else 1)
            out[ring, "frames"] = pl.place_frames(data, offs, "both")
    for what in ("strands", "frames"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[False, what], out[True, what])), what


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_accumulate(gpu_available, oracle_lib, monkeypatch, shards):
    """The accumulate-only launch of a k-mer-space shard (raw sums and counts out, added over the shards, then the
    finish kernel): the same partial vectors as the ring's, and the oracle's placements within the shard bar."""
    from epik_amd.placer import Placer
    from test_kmer_shard_gpu import _assert_close_to_oracle, _emulated_shards
    db = _run_db(300, seed=31)
    data, offs = _reads(seed=32)
    out = {}
    for ring in (False, True):
        _setup(monkeypatch, "paired", "u16", ring=ring)
        with Placer.from_synth(db, shard_index=1, shard_count=shards) as pl:
            assert _lists(pl, "u16") == (0 if ring else 1)
        out[ring] = _emulated_shards(db, data, offs, shards)
    _assert_close_to_oracle(out[False], oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[False], out[True]))


def test_filtered_layout_keeps_the_ring_unless_asked(gpu_available, oracle_lib, monkeypatch):
    from epik_amd.placer import Placer
    amino = synth.make_db(200, states="amino", kmer_size=3, seed=23, p_present=0.5)
    data, offs = synth.make_reads(500, 120, states="amino", seed=24)
    ref = oracle_lib.Oracle.from_synth(amino).place(data, offs, num_threads=0)
    _setup(monkeypatch, "filtered", "u16")
    with Placer.from_synth(amino) as pl:
        assert _lists(pl, "u16") == 0
        assert_rows_match(*pl.place_packed(data, offs), *ref)
    monkeypatch.setenv("EPIK_AMD_RUN_COUNTS", "lists")
    with Placer.from_synth(amino) as pl:
        assert _lists(pl, "u16") == 1
        assert_rows_match(*pl.place_packed(data, offs), *ref)
