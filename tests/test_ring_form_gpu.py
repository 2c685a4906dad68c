"""The two forms of the run-list ring's chunk descriptors (place_device.hpp, RunListLayout): NEAR -- byte offset and
prepared LDS row address, one buffer resource for the launch, twelve instructions a stage -- and FAR, the line-index
form of posting regions of 4 GB and more; and the 64 slack rows behind the wave's score vector that replace the clamp
of a lane's row where they cost no resident wave (N = 999; N = 1 199, n_pad 1 216, keeps the clamp: db_layout.h,
wave_slack_is_free).

Every read of every case is compared with the CPU oracle: n_rows, branch order, float32 scores as uint32 bits and
k-mer counts must be equal bit for bit (conftest.assert_rows_match; the like-weight ratio goes through a
double-precision 10^x that differs from glibc's pow by ulps and keeps the suite's 1e-5 bar).  The two forms must also
agree with each other byte for byte in everything they write, the ratios included.  The same for the run ring of the
run-coded layouts (8-bit counts, images with explicit-cell lists), whose descriptors take the near form under the same
rule."""
import ctypes

import numpy as np
import pytest

from conftest import assert_rows_match
from epik_amd import synth
from epik_amd.synth import PKDB_VALUE, SynthDB

pytestmark = pytest.mark.gpu

COUNTS = {"u16": ("0", 1), "u32": ("1", 2)}  # EPIK_AMD_WIDE_COUNTS, epik_amd::CountBits
NEAR, SLACK = 1, 2                           # EPIK_AMD_RING_NEAR, EPIK_AMD_RING_SLACK
K = 5
AMBIGUOUS = "ACGT" * 3 + "N" + "ACGGT" * 20 + "R" + "TTGCA" * 10


def _db(num_branches, lens, starts, seed):
    """One run per code: code c holds branches starts[c] .. starts[c] + lens[c] - 1."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    assert lens.size == 4 ** K and (lens >= 1).all() and (starts >= 0).all() and (starts + lens <= num_branches).all()
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    values = np.empty(int(offsets[-1]), dtype=PKDB_VALUE)
    key = np.repeat(np.arange(lens.size), lens)
    within = np.arange(values.size) - (np.cumsum(lens) - lens)[key]
    values["branch"] = (starts[key] + within).astype(np.uint32)
    threshold = synth.alphabet.score_threshold(1.5, K, 4)
    values["score"] = np.log10(threshold + rng.random(values.size) * (1.0 - threshold)).astype(np.float32)
    return SynthDB(states="nucl", kmer_size=K, omega=1.5, num_branches=num_branches, offsets=offsets, values=values,
                   threshold=threshold)


def _random_reads(seed, n=200):
    rng = np.random.default_rng(seed)
    reads = ["".join(rng.choice(list("ACGT"), size=int(m))) for m in rng.integers(K, 260, size=n)]
    reads += ["".join(rng.choice(list("ACGT"), size=900)), AMBIGUOUS, "ACG", ""]
    return reads


def _case_synth(num_branches):
    """(a) synth.make_db: the benchmark's own database model and reads, and an ambiguous k-mer (d)."""
    db = synth.make_db(num_branches, kmer_size=6, seed=num_branches, p_present=0.6)
    data, offs = synth.make_reads(1500, 150, seed=num_branches + 1)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    return db, synth.pack_reads(reads + [AMBIGUOUS])


def _case_last_branch(num_branches):
    """(b) every list ends at the last branch: the lanes behind a chunk's end address the rows past the vector -- with
    the slack rows, row base + 63 runs up to 38 rows into them (N = 999, n_pad 1 024: a last chunk of one posting at
    row 998 has its lanes at rows 998 .. 1 061); with the clamp they all land on the dummy row."""
    rng = np.random.default_rng(num_branches + 7)
    lens = np.minimum(rng.choice(np.asarray([1, 2, 3, 38, 39, 63, 64, 65, 66, 129, 130, 200, 257]), size=4 ** K), num_branches)
    db = _db(num_branches, lens, num_branches - lens, seed=num_branches + 8)
    return db, synth.pack_reads(_random_reads(num_branches + 9))


def _case_chunk_counts(num_branches):
    """(c) reads of exactly 1 .. 7, 8, 9, 192 and 193 chunks in their one pass: AAAAA and the four k-mers between a run
    of A and a run of C have one chunk each, CCCCC has two, so "A" * a + "C" * c streams a + 2 c - 8 chunks (a - 4
    without C) -- an empty ring loop (the first trip and the tail alone), exactly one trip, a tail of one, a full round
    of 192, and a second round of one chunk."""
    rng = np.random.default_rng(num_branches + 17)
    lens = rng.integers(1, 65, size=4 ** K)
    code = lambda s: int("".join(str("ACGT".index(ch)) for ch in s), 4)
    lens[code("CCCCC")] = 100
    starts = (rng.random(4 ** K) * (num_branches - lens + 1)).astype(np.int64)
    starts[code("AAAAA")] = num_branches - lens[code("AAAAA")]  # its lanes past the end run off the vector every stage
    db = _db(num_branches, lens, starts, seed=num_branches + 18)
    chunks = lambda s: sum(int(-(-lens[code(s[i:i + K])] // 64)) for i in range(len(s) - K + 1))
    reads = ["A" * (K - 1 + n) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9)] + ["A" * 168 + "C" * 16, "A" * 167 + "C" * 17]
    assert [chunks(r) for r in reads] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 192, 193]
    # the same reads again behind each other and between others: a wave places them one after another
    return db, synth.pack_reads(reads + _random_reads(num_branches + 19, n=40) + reads[::-1] + [AMBIGUOUS])


CASES = {"synth": _case_synth, "last_branch": _case_last_branch, "chunk_counts": _case_chunk_counts}


def _setup(monkeypatch, counts, form):
    for var in ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "paired")
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", COUNTS[counts][0])
    monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", "2")  # a wave places several reads one after another
    monkeypatch.setenv("EPIK_AMD_RING_FORM", form)


def _place(db, data, offs, counts):
    from epik_amd.placer import Placer
    with Placer.from_synth(db, keep_at_most=7) as pl:
        lists, form = ctypes.c_uint32(7), ctypes.c_uint32(7)
        assert pl._lib.epik_amd_placer_run_counts(pl._handle, COUNTS[counts][1], ctypes.byref(lists)) == 0
        assert pl._lib.epik_amd_placer_ring_form(pl._handle, COUNTS[counts][1], ctypes.byref(form)) == 0
        assert lists.value == 1, "the case's database must take the list-counts kernel"
        return pl.place_packed(data, offs), form.value


@pytest.mark.parametrize("form", ["near", "far"])
@pytest.mark.parametrize("counts", ["u16", "u32"])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("num_branches", [999, 1199])
def test_ring_forms_equal_the_oracle(gpu_available, oracle_lib, monkeypatch, num_branches, case, counts, form):
    assert gpu_available
    db, (data, offs) = CASES[case](num_branches)
    ref = oracle_lib.Oracle.from_synth(db, keep_at_most=7).place(data, offs, num_threads=0)
    _setup(monkeypatch, counts, form)
    got, taken = _place(db, data, offs, counts)
    # near with the slack rows at N = 999 (they fit the LDS granules the workgroup occupies anyway, 16- and 32-bit
    # counts alike), near with the clamp at N = 1 199 (256 B more a wave would cost two of its waves a CU), far as asked
    assert taken == (0 if form == "far" else NEAR | SLACK if num_branches == 999 else NEAR), taken
    worst = assert_rows_match(*got, *ref)
    print(f"N = {num_branches} {case} {counts} {form}: {len(offs) - 1} reads, max |dLWR| = {worst:.3e}")


@pytest.mark.parametrize("counts", ["u16", "u32"])
@pytest.mark.parametrize("num_branches", [999, 1199])
def test_ring_forms_write_the_same_bytes(gpu_available, monkeypatch, num_branches, counts):
    assert gpu_available
    for case in sorted(CASES):
        db, (data, offs) = CASES[case](num_branches)
        out = {}
        for form in ("near", "far"):
            _setup(monkeypatch, counts, form)
            out[form], _ = _place(db, data, offs, counts)
        for a, b in zip(out["near"], out["far"]):
            assert a.tobytes() == b.tobytes(), case


def _mixed_db(num_branches):
    """Most lists runs, every seventh one a scattered set of branches (explicit cells): the run ring with both arms."""
    rng = np.random.default_rng(num_branches + 27)
    lens = np.minimum(rng.choice(np.asarray([1, 2, 63, 64, 65, 128, 129, 200]), size=4 ** K), num_branches).astype(np.int64)
    starts = (rng.random(4 ** K) * (num_branches - lens + 1)).astype(np.int64)
    starts[::5] = num_branches - lens[::5]
    db = _db(num_branches, lens, starts, seed=num_branches + 28)
    offsets = db.offsets.astype(np.int64)
    for code in range(0, 4 ** K, 7):
        n = int(lens[code])
        db.values["branch"][offsets[code]:offsets[code] + n] = np.sort(rng.choice(num_branches, size=n, replace=False))
    return db


@pytest.mark.parametrize("counts,mixed", [("u8", False), ("u8", True), ("u16", True), ("u32", True)])
@pytest.mark.parametrize("num_branches", [999, 1199])
def test_run_ring_forms_equal_the_oracle(gpu_available, oracle_lib, monkeypatch, num_branches, counts, mixed):
    """The run ring (8-bit counts, or an image with explicit-cell lists among its runs) with near and far descriptors:
    both equal the oracle, and each other byte for byte."""
    from epik_amd.placer import Placer
    assert gpu_available
    db = _mixed_db(num_branches) if mixed else _case_last_branch(num_branches)[0]
    data, offs = synth.pack_reads(_random_reads(num_branches + 29) + ["A" * 40, "AC" * 100])
    ref = oracle_lib.Oracle.from_synth(db, keep_at_most=7).place(data, offs, num_threads=0)
    width = {"u8": ("2", 0), "u16": ("0", 1), "u32": ("1", 2)}[counts]
    out = {}
    for form in ("near", "far"):
        _setup(monkeypatch, "u16", form)
        monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", width[0])
        with Placer.from_synth(db, keep_at_most=7) as pl:
            lists, taken = ctypes.c_uint32(7), ctypes.c_uint32(7)
            assert pl._lib.epik_amd_placer_run_counts(pl._handle, width[1], ctypes.byref(lists)) == 0
            assert pl._lib.epik_amd_placer_ring_form(pl._handle, width[1], ctypes.byref(taken)) == 0
            assert lists.value == 0, "the run ring is what this case is about"
            assert taken.value == (NEAR if form == "near" else 0)
            out[form] = pl.place_packed(data, offs)
        assert_rows_match(*out[form], *ref)
    for a, b in zip(out["near"], out["far"]):
        assert a.tobytes() == b.tobytes()
