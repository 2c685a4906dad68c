"""The double-precision tail of a read in a kernel of its own (EPIK_AMD_TAIL=kernel: the kernels with list counts stop
behind the rank, finish_rows_kernel -- tail_kernel.hip -- computes 10^score, the LWRs and the filter with a lane per
reported row) against the tail in the wave (EPIK_AMD_TAIL=wave), one library, two handles, the same inputs.

The instrument is byte equality: the row, n_rows and k-mer-count buffers go to the device poisoned (0xA5) and come
back whole, so that what the two forms write AND what they leave alone -- every slot past n_rows -- is compared.  One
case of each group is also held against the CPU oracle with the bars of the parity tests (conftest.assert_rows_match).
Every test asks the handle which kernels it runs (run_counts, ring_form, table_form, tail_form) before it trusts a
comparison.

Databases: synth.make_db without `scattered` (every list a run), k = 6, on a tree of 16 leaves (N = 31: one trip of
the epilogue's sweeps, fewer branches than rows kept at keep_at_most = 64) and on N = 999 (the headline's tree)."""
import ctypes

import numpy as np
import pytest

from conftest import assert_rows_match
from epik_amd import capi, synth

pytestmark = pytest.mark.gpu

K = 6
COUNTS = {"u16": ("0", 1), "u32": ("1", 2)}   # EPIK_AMD_WIDE_COUNTS, epik_amd::CountBits
WAVE, KERNEL = capi.TAIL_WAVE, capi.TAIL_KERNEL
TABLE = {"paired": 2, "tripled": 3}            # EPIK_AMD_TABLE_PAIRED, EPIK_AMD_TABLE_TRIPLED
TOO_NARROW = capi.ROWS_COUNTS_TOO_NARROW
AMBIGUOUS = "ACGT" * 3 + "N" + "ACGGT" * 20 + "R" + "TTGCA" * 10
POISON = 0xA5


@pytest.fixture(scope="module")
def small_db():
    return synth.make_db(synth.make_tree(16, seed=3).num_nodes, kmer_size=K, seed=5, p_present=0.6)


@pytest.fixture(scope="module")
def headline_tree_db():
    return synth.make_db(999, kmer_size=K, seed=6, p_present=0.6)


def _env(monkeypatch, tail, counts="u16", layout="paired"):
    for var in ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_RING_FORM", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    monkeypatch.setenv("EPIK_AMD_LAYOUT", layout)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", COUNTS[counts][0])
    monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", "2")  # a wave places several reads one after another
    monkeypatch.setenv("EPIK_AMD_TAIL", tail)


def _forms(pl, counts):
    """What the handle says it runs for that count width."""
    lib, h, width = pl._lib, pl._handle, COUNTS[counts][1]
    out = {}
    for name, args in (("run_counts", (width,)), ("ring_form", (width,)), ("table_form", ()), ("tail_form", (width,))):
        v = ctypes.c_uint32(99)
        capi.check(getattr(lib, "epik_amd_placer_" + name)(h, *args, ctypes.byref(v)))
        out[name] = int(v.value)
    return out


def _placer(monkeypatch, db, tail, counts="u16", layout="paired", expect=None, **kw):
    """A handle created under the switches, checked to be the instantiation the test means: list counts, the near
    ring, the table asked for, and the tail form `expect` (by default the one asked for)."""
    from epik_amd.placer import Placer
    _env(monkeypatch, tail, counts, layout)
    pl = Placer.from_synth(db, **kw)
    forms = _forms(pl, counts)
    assert forms["run_counts"] == 1, forms
    assert forms["ring_form"] & 1, forms
    assert forms["table_form"] == TABLE[layout], forms
    assert forms["tail_form"] == ({"wave": WAVE, "kernel": KERNEL}[tail] if expect is None else expect), forms
    return pl


class Batch:
    """Reads on the device and poisoned output buffers; run() places and returns everything that came back, whole."""

    def __init__(self, data, offs, keep, with_counts=True):
        import torch
        self.torch = torch
        dev = torch.device("cuda", 0)
        self.n, self.keep = len(offs) - 1, keep
        self.d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        self.d_offs = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).to(dev)
        self.d_rows = torch.empty(self.n * keep * capi.PLACEMENT.itemsize, dtype=torch.uint8, device=dev)
        self.d_n = torch.empty(self.n * 4, dtype=torch.uint8, device=dev)
        self.d_counts = torch.empty(self.n * keep * 4, dtype=torch.uint8, device=dev) if with_counts else None

    def poison(self):
        for t in (self.d_rows, self.d_n, self.d_counts):
            if t is not None:
                t.fill_(POISON)

    def back(self):
        self.torch.cuda.synchronize()
        rows = self.d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(self.n, self.keep)
        n_rows = self.d_n.cpu().numpy().view(np.uint32)
        counts = self.d_counts.cpu().numpy().view(np.uint32).reshape(self.n, self.keep) if self.d_counts is not None else None
        return rows, n_rows, counts

    def run(self, pl, n=None, stream=0):
        self.poison()
        self.torch.cuda.synchronize()
        pl.place_device(self.d_seqs.data_ptr(), self.d_offs.data_ptr(), self.n if n is None else n, self.d_rows.data_ptr(),
                        self.d_n.data_ptr(), self.d_counts.data_ptr() if self.d_counts is not None else 0, stream)
        return self.back()


def _same_bytes(a, b, what):
    for name, x, y in zip(("rows", "n_rows", "kmer_counts"), a, b):
        if x is None and y is None:
            continue
        if x.tobytes() != y.tobytes():
            bad = np.nonzero((x.reshape(len(x), -1).view(np.uint8) != y.reshape(len(y), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differ at reads {bad[:10]} ({len(bad)} of {len(x)})")


def _untouched_past_n_rows(got):
    """Nothing writes a slot past n_rows: the poison is still there, in the rows and in the k-mer counts."""
    rows, n_rows, counts = got
    keep = rows.shape[1]
    past = np.arange(keep)[None, :] >= np.where(n_rows == TOO_NARROW, 0, n_rows).astype(np.int64)[:, None]
    assert (rows.view(np.uint8).reshape(len(rows), keep, -1)[past] == POISON).all()
    if counts is not None:
        assert (counts.view(np.uint8).reshape(len(rows), keep, -1)[past] == POISON).all()


def _valid(got):
    """The rows up to n_rows (and the counts with them), zero elsewhere: what the oracle's arrays look like."""
    rows, n_rows, counts = got
    keep = rows.shape[1]
    valid = np.arange(keep)[None, :] < np.where(n_rows == TOO_NARROW, 0, n_rows).astype(np.int64)[:, None]
    r, c = np.zeros_like(rows), np.zeros_like(counts)
    r[valid], c[valid] = rows[valid], counts[valid]
    return r, n_rows, c


def _code_read(code):
    return "".join("ACGT"[(code >> (2 * (K - 1 - j))) & 3] for j in range(K))


def _kinds(db):
    """One read of every kind the finishing kernel meets: {name: read}."""
    lens = np.diff(db.offsets.astype(np.int64))
    absent, short_list = np.nonzero(lens == 0)[0], np.nonzero((lens >= 1) & (lens <= 3))[0]
    assert len(absent) and len(short_list), "the database must have an absent code and a list of at most three postings"
    rng = np.random.default_rng(77)
    return {"too_short": "ACG",
            "no_list": _code_read(int(absent[0])),                         # one k-mer, absent: rows at the threshold score
            "few_branches": _code_read(int(short_list[0])),                # one k-mer, fewer than keep branches
            "ambiguous": AMBIGUOUS,
            "ordinary": "".join(rng.choice(list("ACGT"), size=150)),
            "too_narrow": "".join(rng.choice(list("ACGT"), size=32767 + K + 3))}  # more k-mers than 16-bit counts hold


@pytest.mark.parametrize("keep", [1, 7, 8, 9, 64])
def test_group_seams(gpu_available, small_db, monkeypatch, keep):
    """Groups of 1, 8, 8, 16 and 64 lanes, batches that end inside a group's wave, at its end and one read behind it."""
    assert gpu_available
    kinds = _kinds(small_db)
    rng = np.random.default_rng(keep)
    reads = [kinds["ordinary"], kinds["no_list"], kinds["few_branches"], kinds["too_short"]]
    reads += ["".join(rng.choice(list("ACGT"), size=int(m))) for m in rng.integers(K, 200, size=61)]
    data, offs = synth.pack_reads(reads)
    batch = Batch(data, offs, keep)
    with _placer(monkeypatch, small_db, "wave", keep_at_most=keep) as wave, \
            _placer(monkeypatch, small_db, "kernel", keep_at_most=keep) as kern:
        for n in (1, 7, 8, 9, 63, 64, 65):
            a, b = batch.run(wave, n), batch.run(kern, n)
            _same_bytes(a, b, f"keep {keep}, {n} reads")
            assert (b[1][n:] == POISON * 0x01010101).all(), "reads behind the batch are not the launch's"
            _untouched_past_n_rows(tuple(x[:n] for x in b))
            assert n < 2 or b[1][1] == keep, "the read without a list reports keep_at_most rows"


def test_no_handle_keeps_more_rows_than_a_wave_has_lanes(gpu_available, small_db, monkeypatch):
    """keep_at_most = 65 would have no group of lanes in the finishing kernel and would have to keep the tail in the wave
    (place_kernel.h: kTailMaxKeep; capi.hip latches the wave form for it).  No such handle exists: create() refuses more
    than 64 rows a read, whatever EPIK_AMD_TAIL says.  Whoever lifts that limit meets this test and owes the wave form
    its report."""
    assert gpu_available
    from epik_amd.placer import Placer
    for tail in ("wave", "kernel"):
        _env(monkeypatch, tail)
        with pytest.raises(capi.EpikAmdError, match=r"keep_at_most must be in \[1, 64\]"):
            Placer.from_synth(small_db, keep_at_most=65)


@pytest.mark.parametrize("counts", ["u16", "u32"])
def test_mixed_kinds_in_one_wave(gpu_available, oracle_lib, small_db, monkeypatch, counts):
    """Reads of every kind next to each other in read order, so that one wave of the finishing kernel (eight reads at
    keep_at_most = 7) holds them all: too short (n_rows 0), too many k-mers for the counts (n_rows stays
    EPIK_AMD_ROWS_COUNTS_TOO_NARROW; 16-bit counts only), no list found, fewer branches than rows kept, an ambiguous
    character, ordinary ones."""
    assert gpu_available
    kinds = _kinds(small_db)
    order = ["too_short", "too_narrow", "no_list", "few_branches", "ambiguous", "ordinary", "too_narrow", "too_short",
             "ordinary", "no_list", "too_short", "few_branches", "too_narrow", "ambiguous", "ordinary", "ordinary", "too_short"]
    data, offs = synth.pack_reads([kinds[k] for k in order])
    ref = oracle_lib.Oracle.from_synth(small_db, keep_at_most=7).place(data, offs, num_threads=0)
    batch = Batch(data, offs, 7)
    with _placer(monkeypatch, small_db, "wave", counts, keep_at_most=7) as wave, \
            _placer(monkeypatch, small_db, "kernel", counts, keep_at_most=7) as kern:
        a, b = batch.run(wave), batch.run(kern)
    _same_bytes(a, b, counts)
    _untouched_past_n_rows(b)
    n_rows = b[1]
    narrow = np.array([k == "too_narrow" for k in order])
    if counts == "u16":
        assert (n_rows[narrow] == TOO_NARROW).all(), n_rows
    assert (n_rows[[k == "too_short" for k in order]] == 0).all(), n_rows
    assert (n_rows[[k == "no_list" for k in order]] == 7).all(), n_rows
    few = n_rows[[k == "few_branches" for k in order]]
    assert (few >= 1).all() and (few <= 3).all(), n_rows
    placed = ~narrow if counts == "u16" else np.ones(len(order), dtype=bool)
    got = _valid(b)
    assert_rows_match(*(x[placed] for x in got), *(x[placed] for x in ref))


@pytest.mark.parametrize("counts", ["u16", "u32"])
def test_the_three_sum_regimes(gpu_available, oracle_lib, small_db, monkeypatch, counts):
    """sum_scores relative to its largest term (ref_score > -280), term by term in double (down to -325) and nothing to
    add below that (score_sum == 0: keep_factor becomes 0 and every row stays, with a ratio of 0) -- reads long enough
    that their threshold score, n_kmers * log10(threshold) / k, crosses both limits, as the reads of
    test_configs_gpu.test_protein_reads_across_the_underflow_limits do."""
    assert gpu_available
    per_kmer = float(small_db.log_threshold) / K
    # (threshold scores from -250 to -690: the best row of such a read lies at about 0.7 of its threshold score)
    lengths = np.repeat((np.arange(-250.0, -700.0, -10.0) / per_kmer).astype(np.int64) + K - 1, 3)
    rng = np.random.default_rng(91)
    data, offs = synth.pack_reads(["".join(rng.choice(list("ACGT"), size=int(m))) for m in lengths])
    ref = oracle_lib.Oracle.from_synth(small_db, keep_at_most=7).place(data, offs, num_threads=0)
    best = ref[0]["score"][:, 0]
    sides = int((best > -280).sum()), int(((best < -280) & (best > -325)).sum()), int((best < -325).sum())
    assert min(sides) >= 9, f"the reads must fall on all three sides of the two limits: {sides}"
    lwr0 = ref[0]["lwr"][:, 0]
    assert (lwr0 == 0).any() and (lwr0 > 0).any()
    batch = Batch(data, offs, 7)
    with _placer(monkeypatch, small_db, "wave", counts, keep_at_most=7) as wave, \
            _placer(monkeypatch, small_db, "kernel", counts, keep_at_most=7) as kern:
        a, b = batch.run(wave), batch.run(kern)
    _same_bytes(a, b, counts)
    _untouched_past_n_rows(b)
    worst = assert_rows_match(*_valid(b), *ref)
    print(f"{counts}: reads on the three sides {sides}, max |dLWR| = {worst:.3e}")


@pytest.mark.parametrize("with_counts", [True, False])
@pytest.mark.parametrize("counts,layout", [("u16", "tripled"), ("u32", "tripled"), ("u16", "paired")])
def test_filter_compacts_rows_and_counts(gpu_available, oracle_lib, headline_tree_db, monkeypatch, counts, layout, with_counts):
    """keep_factor = 0.5 on the headline's tree, the headline's instantiation among the three: the filter cuts the
    ranking anywhere between its first and last row, the kept rows and their k-mer counts land in slots 0 .. n_rows - 1
    -- with the k-mer-count pointer and without it."""
    assert gpu_available
    db = headline_tree_db
    data, offs = synth.make_reads(300, 60, seed=13)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)] + [AMBIGUOUS, "ACG", ""]
    data, offs = synth.pack_reads(reads)
    batch = Batch(data, offs, 7, with_counts)
    with _placer(monkeypatch, db, "wave", counts, layout, keep_at_most=7, keep_factor=0.5) as wave, \
            _placer(monkeypatch, db, "kernel", counts, layout, keep_at_most=7, keep_factor=0.5) as kern:
        a, b = batch.run(wave), batch.run(kern)
    _same_bytes(a, b, f"{counts} {layout} counts {with_counts}")
    _untouched_past_n_rows(b)
    seen = set(int(v) for v in b[1])
    assert len(seen & {1, 2, 3, 4, 5, 6}) >= 3 and 0 in seen, f"the filter must cut the ranking at several places: {sorted(seen)}"
    if with_counts and counts == "u16" and layout == "tripled":
        ref = oracle_lib.Oracle.from_synth(db, keep_at_most=7, keep_factor=0.5).place(data, offs, num_threads=0)
        assert_rows_match(*_valid(b), *ref)


def test_one_handle_several_calls_and_two_streams(gpu_available, small_db, monkeypatch):
    """n = 9, then 65, then 9 on one handle: the workspace grows and is used again.  Then a place launch and the finish
    launch of a dense k-mer-space shard (finish_reads_kernel: the tail in its wave, no workspace) on two streams at
    once, each compared with the same launch by itself."""
    assert gpu_available
    import torch
    rng = np.random.default_rng(5)
    reads = ["".join(rng.choice(list("ACGT"), size=int(m))) for m in rng.integers(K, 200, size=63)] + [AMBIGUOUS, "ACG"]
    data, offs = synth.pack_reads(reads)
    n, N = len(reads), small_db.num_branches
    batch = Batch(data, offs, 7)
    with _placer(monkeypatch, small_db, "wave", keep_at_most=7) as wave, _placer(monkeypatch, small_db, "kernel", keep_at_most=7) as kern:
        for m in (9, 65, 9):
            _same_bytes(batch.run(wave, m), batch.run(kern, m), f"{m} reads")
        # the halves of a one-shard placement: accumulate, then finish on the sums
        dev = torch.device("cuda", 0)
        d_scores = torch.zeros(n * N, dtype=torch.float32, device=dev)
        d_counts = torch.zeros(n * N, dtype=torch.int16, device=dev)
        kern.accumulate_device(batch.d_seqs.data_ptr(), batch.d_offs.data_ptr(), n, d_scores.data_ptr(), d_counts.data_ptr())
        torch.cuda.synchronize()
        other = Batch(data, offs, 7)
        s_place, s_finish = torch.cuda.Stream(), torch.cuda.Stream()

        def finish(stream):
            kern.finish_device(other.d_offs.data_ptr(), n, d_scores.data_ptr(), d_counts.data_ptr(), other.d_rows.data_ptr(),
                               other.d_n.data_ptr(), other.d_counts.data_ptr(), stream.cuda_stream)

        placed_alone = batch.run(kern, stream=s_place.cuda_stream)
        other.poison()
        torch.cuda.synchronize()
        finish(s_finish)
        finished_alone = other.back()
        batch.poison(), other.poison()
        torch.cuda.synchronize()
        kern.place_device(batch.d_seqs.data_ptr(), batch.d_offs.data_ptr(), n, batch.d_rows.data_ptr(), batch.d_n.data_ptr(),
                          batch.d_counts.data_ptr(), s_place.cuda_stream)
        finish(s_finish)
        _same_bytes(batch.back(), placed_alone, "place beside finish")
        _same_bytes(other.back(), finished_alone, "finish beside place")
        _same_bytes(placed_alone, batch.run(wave), "place, kernel against wave")
        # (the two halves give the rows of the one-pass placement)
        v_place, v_finish = _valid(placed_alone), _valid(finished_alone)
        assert v_place[1].tobytes() == v_finish[1].tobytes() and v_place[0]["branch"].tobytes() == v_finish[0]["branch"].tobytes()
