"""The abundance profile on the GPU (epik_amd_profile_*, epik_amd_placer_profile_*, Placer.profile, epik-dna --profile /
--profile-only): the device sums against the rule of include/epik_amd.h written out here in numpy -- bit for bit on the
rows the placement wrote and on forged rows, at the default keep_at_most and at six others, within the project's LWR bar
against the CPU oracle's rows --, the same bits whatever the pieces, the grid, the path or the chunks, and the drivers'
files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_rows_match, mixed_reads, select_kernel
from epik_amd import capi, dbfile, synth
from test_strand_gpu import KERNELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LWR_BITS = 30
TOO_NARROW = 0xFFFFFFFF
U64 = np.uint64
#: beside the kernels of the strand tests on the small tree: the streaming kernels of large trees, the accumulators
#: in LDS beside other workgroups' (N = 2 999) or a workgroup per CU (N = 3 999), and a tree whose accumulators exceed
#: the LDS path (N = 10 399)
LARGE = {"tree2999": 1500, "tree3999": 2000, "tree10399": 5200}
LDS_LIMIT = 160 * 1024 - 64


def q(lwr):
    """llrint(x * 2^30), round half to even."""
    return np.rint(np.asarray(lwr, dtype=np.float64) * np.float64(1 << LWR_BITS)).astype(np.int64).astype(U64)


def numpy_rule(rows, n_rows, counts, weights, num_branches):
    """The table of the rule over whole arrays; uint64 arithmetic wraps modulo 2^64 as the accumulators do."""
    n, keep = rows.shape
    w = (np.ones(n, U64) if weights is None else np.asarray(weights).astype(U64))
    narrow, short = n_rows == TOO_NARROW, n_rows == 0
    no_hit = ~narrow & ~short & (counts[:, 0] == 0)
    placed = ~narrow & ~short & ~no_hit
    valid = placed[:, None] & (np.arange(keep, dtype=np.int64)[None, :] < n_rows.astype(np.int64)[:, None])
    bad = valid & (rows["branch"] >= num_branches)
    ok = valid & ~bad
    totals = {name: int(w[m].sum(dtype=U64)) for name, m in
              (("placed", placed), ("no_hit", no_hit), ("too_short", short), ("too_narrow", narrow))}
    totals["bad_rows"] = int(bad.sum())
    mass, best = np.zeros(num_branches, U64), np.zeros(num_branches, U64)
    w_rows = np.broadcast_to(w[:, None], (n, keep))
    np.add.at(mass, rows["branch"][ok], w_rows[ok] * q(rows["lwr"][ok]))
    np.add.at(best, rows["branch"][:, 0][ok[:, 0]], w[ok[:, 0]])
    return mass, best, totals


def assert_profile(got, want, what=""):
    mass, best, totals = want
    assert got.totals == totals, (what, got.totals, totals)
    assert np.array_equal(got.best, best), (what, np.nonzero(got.best != best)[0][:10])
    assert np.array_equal(got.mass, mass), (what, np.nonzero(got.mass != mass)[0][:10])


@pytest.fixture(params=KERNELS + sorted(LARGE))
def case(request, monkeypatch, small_case):
    """(name, tree, db): a kernel of the strand tests on the small tree, or a large tree with the kernels create() picks."""
    if request.param in LARGE:
        for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
            monkeypatch.delenv(var, raising=False)
        tree = synth.make_tree(LARGE[request.param], seed=30)
        return request.param, tree, synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    select_kernel(monkeypatch, request.param)
    return (request.param,) + tuple(small_case)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _reads(k, rng, n=600):
    reads = mixed_reads(rng, n, k, alphabet_amb="ACGTNRYKMSWBDHV-", max_len=200)
    reads = [r.lower() if i % 7 == 0 else r for i, r in enumerate(reads)]
    return reads + ["ACG", "", "NNNNNNNNNN", "-" * 12]


class DeviceBatch:
    """Reads placed with place_device into torch buffers that stay on the device."""

    def __init__(self, pl, reads, weights=None):
        import torch
        self.torch, self.pl = torch, pl
        data, offs = synth.pack_reads(reads)
        dev = torch.device("cuda", pl.device)
        self.n, keep = len(reads), pl.keep_at_most
        self.d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
        self.d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
        # (poisoned: the slots past n_rows keep this garbage, which the profile must not look at)
        self.d_rows = torch.full((self.n * keep * 2,), float("nan"), dtype=torch.float64, device=dev)
        self.d_n = torch.zeros(self.n, dtype=torch.int32, device=dev)
        self.d_counts = torch.full((self.n * keep,), 3, dtype=torch.int32, device=dev)
        self.weights = weights
        self.d_w = None if weights is None else torch.from_numpy(np.asarray(weights, np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize()
        self.stream = torch.cuda.Stream()
        pl.place_device(self.d_seqs.data_ptr(), self.d_offs.data_ptr(), self.n, self.d_rows.data_ptr(), self.d_n.data_ptr(),
                        self.d_counts.data_ptr(), self.stream.cuda_stream)
        self.stream.synchronize()

    def host(self):
        keep = self.pl.keep_at_most
        return (self.d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(self.n, keep), self.d_n.cpu().numpy().view(np.uint32),
                self.d_counts.cpu().numpy().view(np.uint32).reshape(self.n, keep))

    def add_to(self, profile, first=0, count=None, stream=None):
        count = self.n - first if count is None else count
        keep = self.pl.keep_at_most
        stream = self.stream if stream is None else stream
        profile.add_device(self.d_rows.data_ptr() + first * keep * 16, self.d_n.data_ptr() + first * 4,
                           self.d_counts.data_ptr() + first * keep * 4, count,
                           0 if self.d_w is None else self.d_w.data_ptr() + first * 4, stream.cuda_stream)


def _four_class_batch(pl, k, rng):
    """Reads of all four classes and the count width that makes some of them too narrow: 8-bit counts and a read of more
    than 255 k-mers, or, where the handle has no 8-bit kernel, the default 16 bits and one of more than 32 767."""
    reads = _reads(k, rng, 500)
    if pl._lib.epik_amd_placer_set_wide_counts(pl._handle, 2) == capi.OK:
        reads = [r[:200] for r in reads] + ["".join(rng.choice(list("ACGT"), size=300)) for _ in range(3)]
    else:
        capi.check(pl._lib.epik_amd_placer_set_wide_counts(pl._handle, 0))
        reads += ["".join(rng.choice(list("ACGT"), size=33_000)) for _ in range(2)]
    reads += ["ACGTTGCA"] * (3 if len(reads) % 64 == 61 else 0)
    rng.shuffle(reads)
    weights = rng.integers(0, 5, size=len(reads)).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    return reads, weights


def test_add_device_equals_the_rule_on_the_rows_just_written(placer_cls, case):
    _, _, db = case
    rng = np.random.default_rng(11)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        reads, weights = _four_class_batch(pl, db.kmer_size, rng)
        assert len(reads) % 64 != 0
        batch = DeviceBatch(pl, reads, weights)
        batch.add_to(profile)
        got = profile.read()
        rows, n_rows, counts = batch.host()
        want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
        assert_profile(got, want)
        totals = want[2]
        assert min(totals["placed"], totals["no_hit"], totals["too_short"], totals["too_narrow"]) > 0 and totals["bad_rows"] == 0
        assert profile.lds_path == (16 * db.num_branches <= LDS_LIMIT)
        # without weights every read counts once; reset() empties the profile
        profile.reset()
        assert not profile.read().mass.any() and profile.read().records == 0
        unweighted = DeviceBatch(pl, reads)
        unweighted.add_to(profile)
        assert_profile(profile.read(), numpy_rule(rows, n_rows, counts, None, db.num_branches), "no weights")
        assert profile.read().records == len(reads)


def test_profile_of_gpu_rows_against_the_oracle(placer_cls, oracle_lib, case):
    """best and the totals equal the oracle's exactly (scores are bit-exact, ties go to the lower branch); mass within
    what the LWR bar of assert_rows_match (1e-5) allows per row: ceil(1e-5 * 2^30) for the two LWRs and 1 for the two
    roundings, times the weight -- derived from that bar, not measured."""
    _, _, db = case
    reads = _reads(db.kmer_size, np.random.default_rng(1))
    weights = np.random.default_rng(2).integers(0, 5, size=len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    ref = oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        rows, n_rows, counts = pl.place_packed(data, offs)
        assert_rows_match(rows, n_rows, counts, *ref)
        profile.add_host(rows, n_rows, counts, weights)
        got = profile.read()
    mass, best, totals = numpy_rule(*ref, weights, db.num_branches)
    assert got.totals == totals and np.array_equal(got.best, best)
    assert totals["placed"] > 0 and totals["no_hit"] > 0 and totals["too_short"] > 0
    keep = ref[0].shape[1]
    valid = (np.arange(keep)[None, :] < ref[1].astype(np.int64)[:, None]) & (ref[2][:, :1] != 0)
    w_on = np.zeros(db.num_branches, U64)
    np.add.at(w_on, ref[0]["branch"][valid], np.broadcast_to(weights.astype(U64)[:, None], valid.shape)[valid])
    bound = w_on * U64(int(np.ceil(1e-5 * 2 ** 30)) + 1)
    delta = np.abs(got.mass.astype(np.int64) - mass.astype(np.int64)).astype(U64)
    print("max |mass - mass_oracle| =", int(delta.max()), "of a bound of", int(bound[np.argmax(delta)]))
    assert (delta <= bound).all(), np.nonzero(delta > bound)[0][:10]


def test_every_lane_on_the_same_cells(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    read = "ACGTTGCAAGGCTTACGATCGGA"
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        rows, n_rows, counts = pl.place_packed(*synth.pack_reads([read]))
        assert n_rows[0] > 0 and counts[0, 0] > 0
        batch = DeviceBatch(pl, [read] * 100_000)
        batch.add_to(profile)
        got = profile.read()
    want = np.zeros(db.num_branches, U64)
    for j in range(int(n_rows[0])):
        want[rows[0, j]["branch"]] += U64(100_000) * q(rows[0, j]["lwr"])
    assert np.array_equal(got.mass, want)
    assert got.best[rows[0, 0]["branch"]] == 100_000 and int(got.best.sum()) == 100_000
    assert got.totals == dict(placed=100_000, no_hit=0, too_short=0, too_narrow=0, bad_rows=0)


@pytest.mark.parametrize("tree_name", ["small", "tree3999"])
def test_same_bits_whatever_the_pieces_the_grid_and_the_path(placer_cls, small_case, monkeypatch, tree_name):
    import torch
    if tree_name == "small":
        select_kernel(monkeypatch, "paired")
        _, db = small_case
    else:
        for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
            monkeypatch.delenv(var, raising=False)
        tree = synth.make_tree(LARGE[tree_name], seed=30)
        db = synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    rng = np.random.default_rng(21)
    reads = _reads(db.kmer_size, rng, 3000)
    weights = rng.integers(0, 1 << 32, size=len(reads), dtype=np.uint64).astype(np.uint32)
    results = {}
    variants = [("one call", {}), ("uneven pieces", {}), ("two streams", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"}),
                ("global path", {"EPIK_AMD_PROFILE_LDS": "0"})]
    variants.append(("lds path", {"EPIK_AMD_PROFILE_LDS": "1"}))
    for name, env in variants:
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.profile() as profile:
            pl.choose_counts(200)
            batch = DeviceBatch(pl, reads, weights)
            if name == "uneven pieces":
                cuts = [0, 1, 64, 65, 700, 701, 2999, len(reads)]
                for a, b in zip(cuts, cuts[1:]):
                    batch.add_to(profile, a, b - a)
                batch.add_to(profile, 5, 0)            # n == 0: nothing
            elif name == "two streams":
                other = torch.cuda.Stream()
                batch.add_to(profile, 0, 1500)
                batch.add_to(profile, 1500, None, other)
            else:
                batch.add_to(profile)
            results[name] = profile.read()
            if name == "one call":
                want = numpy_rule(*batch.host(), weights, db.num_branches)
            if "EPIK_AMD_PROFILE_LDS" in env:
                assert profile.lds_path == (env["EPIK_AMD_PROFILE_LDS"] == "1")
        for key in env:
            monkeypatch.delenv(key)
    for name, got in results.items():
        assert_profile(got, want, name)


def test_lds_path_is_refused_where_the_cells_do_not_fit(placer_cls, monkeypatch):
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    tree = synth.make_tree(LARGE["tree10399"], seed=30)
    db = synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    assert 16 * db.num_branches > LDS_LIMIT
    monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", "1")
    with placer_cls.from_synth(db) as pl:
        with pytest.raises(capi.EpikAmdError) as e:
            pl.profile()
        assert e.value.code == capi.ERR_UNSUPPORTED


def test_hand_made_rows_move_only_bad_rows(placer_cls, small_case, monkeypatch):
    import torch
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    n_branches = db.num_branches
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        keep = pl.keep_at_most
        rows = np.zeros((130, keep), dtype=capi.PLACEMENT)
        rows["branch"] = 0xFFFFFFF0                       # garbage everywhere, also beyond n_rows
        rows["lwr"] = np.nan
        n_rows = np.full(130, 2, dtype=np.uint32)
        rows["branch"][:, 0] = n_branches                 # the first row just past the tree
        rows["branch"][:, 1] = np.arange(130) + n_branches + 1
        rows["lwr"][:, :2] = 0.5
        counts = np.ones((130, keep), dtype=np.uint32)
        weights = np.full(130, 3, dtype=np.uint32)
        weights[7] = 0                                    # (a bad row counts whatever the read's weight)
        profile.add_host(rows, n_rows, counts, weights)
        got = profile.read()
        assert not got.mass.any() and not got.best.any()
        assert got.totals == dict(placed=int(weights.sum()), no_hit=0, too_short=0, too_narrow=0, bad_rows=260)
        assert got.totals == numpy_rule(rows, n_rows, counts, weights, n_branches)[2]
        # a read with one good and one bad row: the good one is summed
        rows["branch"][3, 0], rows["branch"][4, 1] = 2, 5
        profile.reset()
        profile.add_host(rows, n_rows, counts, weights)
        assert_profile(profile.read(), numpy_rule(rows, n_rows, counts, weights, n_branches))
        assert profile.read().totals["bad_rows"] == 258 and profile.read().best[2] == 3 and profile.read().best[5] == 0
    del torch


def test_profile_reads_and_strands_equal_add_device_over_the_placed_rows(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    _, db = small_case
    rng = np.random.default_rng(31)
    reads = _reads(db.kmer_size, rng, 2500) + ["".join(rng.choice(list("ACGT"), size=40_000))]
    weights = rng.integers(0, 9, size=len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        for strand, env in ((None, "EPIK_AMD_PROFILE_CHUNK_READS"), ("both", "EPIK_AMD_STRAND_CHUNK_READS"),
                            ("reverse", "EPIK_AMD_STRAND_CHUNK_READS")):
            if strand is None:
                rows, n_rows, counts = pl.place_packed(data, offs)
                labels = None
            else:
                rows, n_rows, counts, labels = pl.place_strands(data, offs, strand)
            want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
            profile.reset()
            profile.add_host(rows, n_rows, counts, weights)
            assert_profile(profile.read(), want, f"add_device {strand}")
            profile.reset()
            got_labels = pl.profile_packed(profile, data, offs, weights, strand=strand)
            assert_profile(profile.read(), want, f"profile_packed {strand}")
            assert (got_labels is None) if labels is None else np.array_equal(got_labels, labels)
            monkeypatch.setenv(env, "5")     # chunks of five reads
            profile.reset()
            small = slice(0, 333)
            got_labels = pl.profile_packed(profile, *synth.pack_reads(reads[small]), weights[small], strand=strand)
            monkeypatch.delenv(env)
            assert_profile(profile.read(), numpy_rule(rows[small], n_rows[small], counts[small], weights[small], db.num_branches),
                           f"chunks of 5 {strand}")
            assert labels is None or np.array_equal(got_labels, labels[small])
        # the handle's count state is as place() leaves it, and unweighted reads count once
        profile.reset()
        assert pl.profile_packed(profile, data, offs) is None
        assert profile.read().records == len(reads)
        # a profile of another shape is refused
        with placer_cls.from_synth(db, keep_at_most=3) as other, pytest.raises(capi.EpikAmdError) as e:
            other.profile_packed(profile, data, offs)
        assert e.value.code == capi.ERR_INVALID


def test_profile_frames_equal_add_device_over_the_placed_rows(placer_cls, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT" if i % 3 else "ACGTUNRYKMSWBDHV-."), size=int(rng.integers(0, 200)))) for i in range(700)]
    reads += ["", "AC", "TAATAGTGATAATAGTGA", "NNNNNNNNNNNN"]
    weights = rng.integers(0, 9, size=len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        for chunk in (None, "5"):
            rows, n_rows, counts, frames = pl.place_frames(data, offs, "both")
            want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
            assert want[2]["placed"] > 0 and want[2]["too_short"] > 0
            if chunk:
                monkeypatch.setenv("EPIK_AMD_FRAME_CHUNK_READS", chunk)
            profile.reset()
            got_frames = pl.profile_packed(profile, data, offs, weights, translate="both")
            monkeypatch.delenv("EPIK_AMD_FRAME_CHUNK_READS", raising=False)
            assert_profile(profile.read(), want, f"frames, chunk {chunk}")
            assert np.array_equal(got_frames, frames)
        with pytest.raises(capi.EpikAmdError) as e:          # strands need a nucleotide handle
            pl.profile_packed(profile, data, offs, strand="both")
        assert e.value.code == capi.ERR_UNSUPPORTED


# ---- other keep_at_most ------------------------------------------------------------------------------------------------
#: the kernels map row slot 256 t + lane to (read, row) by a division by keep: other remainders of 256 than 7's
OTHER_KEEPS = (1, 2, 3, 8, 13, 64)
_KEEP_CASE = []


def keep_case():
    """(tree, db) of 79 branches -- enough for 64 rows a read --, k = 4."""
    if not _KEEP_CASE:
        tree = synth.make_tree(40, seed=30)
        _KEEP_CASE.append((tree, synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)))
    return _KEEP_CASE[0]


def forged_rows(rng, n, keep, num_branches):
    """test_cohort_cpu.hand_rows with reads whose n_rows lies beyond keep (every row of theirs counts), more bad rows,
    and weights that include 0 and 0xFFFFFFFF."""
    from test_cohort_cpu import hand_rows
    rows, n_rows, counts = hand_rows(rng, n, keep, num_branches)
    n_rows[4::19] = keep + 5
    rows["branch"][2::7, 0] = num_branches + 1
    weights = rng.integers(0, 4, size=n).astype(np.uint32)
    weights[::11] = 0
    weights[3::29] = 0xFFFFFFFF
    return rows, n_rows, counts, weights


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("keep", OTHER_KEEPS)
def test_profile_at_other_keep_at_most(placer_cls, monkeypatch, keep, lds):
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", lds)
    _, db = keep_case()
    assert db.num_branches == 79
    rng = np.random.default_rng(keep)
    reads = _reads(db.kmer_size, rng, 600)
    weights = rng.integers(0, 5, size=len(reads)).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    weights[-4:] = (1, 2, 3, 0xFFFFFFFF)                    # the fixed reads that end _reads count, whatever the draw
    with placer_cls.from_synth(db, keep_at_most=keep) as pl, pl.profile() as profile:
        assert pl.keep_at_most == keep and profile.lds_path == (lds == "1")
        # the rows the placement has just written
        pl.choose_counts(200)
        batch = DeviceBatch(pl, reads, weights)
        batch.add_to(profile)
        rows, n_rows, counts = batch.host()
        want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
        assert_profile(profile.read(), want, f"placed rows, keep {keep}")
        assert want[2]["placed"] > 0 and want[2]["no_hit"] > 0 and want[2]["too_short"] > 0 and want[2]["bad_rows"] == 0
        # forged rows
        rows, n_rows, counts, weights = forged_rows(rng, 700, keep, db.num_branches)
        want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
        profile.reset()
        profile.add_host(rows, n_rows, counts, weights)
        assert_profile(profile.read(), want, f"forged rows, keep {keep}")
        assert min(want[2].values()) > 0 and ((n_rows == keep + 5) & (counts[:, 0] != 0)).sum() > 0


def test_place_feeds_the_multiplicities(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree, db = small_case
    reads = _reads(db.kmer_size, np.random.default_rng(5), 100)
    records = [(f"r{i}", s) for i, s in enumerate(reads)] + [(f"d{i}", reads[i % 7]) for i in range(40)]
    with placer_cls.from_synth(db, tree) as pl, pl.profile() as profile:
        plain = pl.place(records)
        placed = pl.place(records, profile=profile)
        got = profile.read()
        assert placed == plain
    assert got.records == len(records)
    want = _profile_of_collection(placed, db.num_branches)
    assert_profile(got, want)


def _profile_of_collection(placed, num_branches):
    """The rule over a PlacedCollection: every unique sequence with the number of its headers as weight."""
    mass, best = np.zeros(num_branches, U64), np.zeros(num_branches, U64)
    totals = dict(placed=0, no_hit=0, too_short=0, too_narrow=0, bad_rows=0)
    for seq in placed.placed_seqs:
        w = len(placed.sequence_map[seq.sequence])
        if not seq.placements:
            totals["too_short"] += w
        elif seq.placements[0].count == 0:
            totals["no_hit"] += w
        else:
            totals["placed"] += w
            best[seq.placements[0].branch_id] += U64(w)
            for p in seq.placements:
                mass[p.branch_id] += U64(w) * q(p.weight_ratio)
    return mass, best, totals


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for h, s in records:
            fh.write(f">{h}\n")
            for j in range(0, len(s), 70):
                fh.write(s[j:j + 70] + "\n")


def _expected_tsv(want, tree):
    """The file of the issue, formatted here: prefix-sum free -- every clade by walking up from its members."""
    mass, best, totals = want
    n = tree.num_nodes
    clade_mass, clade_best = [0] * n, [0] * n
    for b in range(n):
        node = b
        while node >= 0:
            clade_mass[node] += int(mass[b])
            clade_best[node] += int(best[b])
            node = int(tree.parent[node])
    records = totals["placed"] + totals["no_hit"] + totals["too_short"]
    lines = [f"# epik_amd profile v1\tlwr_bits=30\trecords={records}\tplaced={totals['placed']}\tno_hit={totals['no_hit']}"
             f"\ttoo_short={totals['too_short']}", "edge_num\tbest\tmass_q\tmass\tclade_best\tclade_mass_q\tclade_mass"]
    for b in range(n):
        lines.append("%d\t%d\t%d\t%.9f\t%d\t%d\t%.9f" % (b, int(best[b]), int(mass[b]), int(mass[b]) / 2.0 ** 30, clade_best[b],
                                                          clade_mass[b], clade_mass[b] / 2.0 ** 30))
    return ("\n".join(lines) + "\n").encode()


def test_drivers_write_the_same_profile_with_and_without_the_jplace(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(500, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=80, ref_length=700, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    data, offs = synth.make_clade_reads(refs, 3000, 150, seed=15)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(3000)]
    rng = np.random.default_rng(16)
    reads += ["".join(rng.choice(list("ACGT"), size=12)) for _ in range(300)]        # three k-mers: mostly without any hit
    reads += [reads[i % 50] for i in range(400)] + ["ACG", "AC", "ACG"]              # duplicated records, too short ones
    records = [(f"read_{i}", s) for i, s in enumerate(reads)]
    fasta = str(tmp_path / "sample.fasta")
    _write_fasta(fasta, records)
    batch = 777
    # what the driver computes: dedup per batch of 777 records (place.cpp:207), here through Placer.place
    want = (np.zeros(db.num_branches, U64), np.zeros(db.num_branches, U64), dict.fromkeys(
        ("placed", "no_hit", "too_short", "too_narrow", "bad_rows"), 0))
    with placer_cls.from_synth(db, tree) as pl:
        for first in range(0, len(records), batch):
            part = _profile_of_collection(pl.place(records[first:first + batch]), db.num_branches)
            want = (want[0] + part[0], want[1] + part[1], {k: want[2][k] + part[2][k] for k in want[2]})
    assert want[2]["placed"] > 0 and want[2]["no_hit"] > 0 and want[2]["too_short"] == 3
    expected = _expected_tsv(want, tree)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    outs = {}
    runs = {"plain": [], "profile": ["--profile"], "only_j1": ["--profile-only", "-j", "1"], "only_j16": ["--profile-only", "-j", "16"],
            "only_two_handles": ["--profile-only", "--devices", "0,0", "-j", "4"],
            "only_both_strands": ["--profile-only", "--strand", "both"], "profile_both_strands": ["--profile", "--strand=both"]}
    for name, extra in runs.items():
        outs[name] = tmp_path / name
        outs[name].mkdir()
        run = subprocess.run([driver, "-d", db_path, "-q", fasta, "-o", str(outs[name]), "--batch-size", str(batch)] + extra,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, name + run.stdout[-2000:] + run.stderr[-2000:]
    tsv = {name: (path / "profile_sample.fasta.tsv") for name, path in outs.items()}
    assert not tsv["plain"].exists()
    for name in ("profile", "only_j1", "only_j16", "only_two_handles"):
        assert tsv[name].read_bytes() == expected, name
        assert (outs[name] / "placements_sample.fasta.jplace").exists() == (name == "profile")
    # the jplace is what it is without --profile: the same bytes, but for the one line that quotes the command line
    # (metadata.invocation: it names the flag and the output directory)
    with_profile = (outs["profile"] / "placements_sample.fasta.jplace").read_bytes().split(b"\n")
    plain = (outs["plain"] / "placements_sample.fasta.jplace").read_bytes().split(b"\n")
    quoted = [i for i, line in enumerate(plain) if b'"invocation"' in line]
    assert len(quoted) == 1 and b"--profile" in with_profile[quoted[0]] and b"--profile" not in plain[quoted[0]]
    del with_profile[quoted[0]], plain[quoted[0]]
    assert with_profile == plain and len(plain) > 3000
    # both strands: the two ways agree with each other, the strands file is written either way
    assert tsv["only_both_strands"].read_bytes() == tsv["profile_both_strands"].read_bytes()
    assert (outs["only_both_strands"] / "strands_sample.fasta.tsv").read_bytes() == (
        outs["profile_both_strands"] / "strands_sample.fasta.tsv").read_bytes()
    # the launcher passes the flag on
    out_l = tmp_path / "launcher"
    out_l.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(out_l),
                          "--profile-only", fasta], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert [p.name for p in out_l.iterdir()] == ["profile_sample.fasta.tsv"]
    from epik_amd import profile as profile_mod
    back = profile_mod.read_tsv(str(out_l / "profile_sample.fasta.tsv"))
    assert back["records"] == len(records) and back["clade_best"][tree.num_nodes - 1] == back["placed"]
