"""A cohort of samples on the GPU (epik_amd_cohort_*, epik_amd_placer_cohort_*, Placer.cohort, epik-dna / epik-aa
--cohort): the cells against the profile's rule applied per sample, bit for bit whatever the grouping of the samples,
the pieces, the grid, the path, the chunks or keep_at_most, bad rows in a workgroup's current sample and in any other
included; the KR distances against the host mirror and the numpy restatement, bit for bit; and the drivers' files."""
import os
import subprocess

import numpy as np
import pytest

from conftest import select_kernel
from epik_amd import capi, cohort as cohort_mod, dbfile, profile as profile_mod, synth
from test_assign_cpu import caterpillar
from test_cohort_cpu import assert_cells, numpy_cohort, numpy_first, numpy_kr, random_cells, same_bits
from test_profile_gpu import LARGE, OTHER_KEEPS, DeviceBatch, _reads, _write_fasta, forged_rows, keep_case
from test_strand_gpu import KERNELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
ENV = ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT")
LDS_LIMIT = 160 * 1024 - 64


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


@pytest.fixture(params=KERNELS + sorted(LARGE))
def case(request, monkeypatch, small_case):
    """(name, db): a kernel of the strand tests on the small tree, or a large tree with the kernels create() picks."""
    if request.param in LARGE:
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        tree = synth.make_tree(LARGE[request.param], seed=30)
        return request.param, synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    select_kernel(monkeypatch, request.param)
    return request.param, small_case[1]


def assignments(n, num_samples):
    """name -> samples[n]: the ways the issue shares the reads out."""
    grouped = (np.arange(n, dtype=np.int64) * num_samples // n).astype(np.uint32)
    out = {"grouped": grouped, "interleaved": (np.arange(n) % num_samples).astype(np.uint32),
           "all in the last": np.full(n, num_samples - 1, dtype=np.uint32)}
    if num_samples > 1:
        empty = num_samples // 2
        rest = (np.arange(n, dtype=np.int64) * (num_samples - 1) // n).astype(np.uint32)
        out["one empty"] = np.where(rest >= empty, rest + 1, rest).astype(np.uint32)
    return out


def device_samples(batch, samples):
    torch = batch.torch
    return torch.from_numpy(np.ascontiguousarray(samples, dtype=np.uint32).view(np.int32)).to(batch.d_n.device)


def add_to(batch, cohort, d_samples, first=0, count=None, stream=None):
    count = batch.n - first if count is None else count
    keep = batch.pl.keep_at_most
    stream = batch.stream if stream is None else stream
    cohort.add_device(batch.d_rows.data_ptr() + first * keep * 16, batch.d_n.data_ptr() + first * 4,
                      batch.d_counts.data_ptr() + first * keep * 4, d_samples.data_ptr() + first * 4, count,
                      0 if batch.d_w is None else batch.d_w.data_ptr() + first * 4, stream.cuda_stream)


def test_add_device_equals_the_profile_rule_per_sample(placer_cls, case):
    _, db = case
    rng = np.random.default_rng(11)
    reads = _reads(db.kmer_size, rng)
    assert len(reads) == 604
    weights = rng.integers(0, 5, size=len(reads)).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        plain, weighted = DeviceBatch(pl, reads), DeviceBatch(pl, reads, weights)
        rows, n_rows, counts = plain.host()
        for num_samples in (1, 3, 40):
            with pl.cohort(num_samples) as cohort:
                assert cohort.lds_path == (16 * db.num_branches <= LDS_LIMIT)
                for name, samples in assignments(len(reads), num_samples).items():
                    d_samples = device_samples(plain, samples)
                    for batch, w in ((plain, None), (weighted, weights)):
                        cohort.reset()
                        add_to(batch, cohort, d_samples)
                        got = cohort.read()
                        want = numpy_cohort(rows, n_rows, counts, w, samples, num_samples, db.num_branches)
                        assert_cells(got, want, (num_samples, name, w is not None))
                        if name == "one empty":
                            e = num_samples // 2
                            assert not got.mass[e].any() and not got.best[e].any() and got.records()[e] == 0
                    if name == "grouped":
                        # the rows summed over the samples are what the profile gives on the same rows
                        profile.reset()
                        weighted.add_to(profile)
                        whole = profile.read()
                        assert np.array_equal(got.mass.sum(axis=0, dtype=U64), whole.mass)
                        assert np.array_equal(got.best.sum(axis=0, dtype=U64), whole.best)
                        for k in ("placed", "no_hit", "too_short", "too_narrow", "bad_rows"):
                            assert int(got.totals[k].sum(dtype=U64)) == whole.totals[k]
        assert whole.totals["placed"] > 0 and whole.totals["no_hit"] > 0 and whole.totals["too_short"] > 0


def _mixed_samples(n, num_samples, rng):
    """Runs of random lengths (a workgroup's LDS sample changes inside its range), a stretch of interleaved reads, some
    reads of no sample."""
    cuts = np.sort(rng.integers(0, n, size=num_samples - 1))
    samples = np.searchsorted(cuts, np.arange(n), side="right").astype(np.uint32)
    samples[n // 2:n // 2 + 90] = rng.integers(0, num_samples, size=90)
    samples[3::97] = num_samples + 5
    samples[n - 1] = 0xFFFFFFFF
    return samples


@pytest.mark.parametrize("tree_name", ["small", "tree3999"])
def test_same_bits_whatever_the_pieces_the_grid_and_the_path(placer_cls, small_case, monkeypatch, tree_name):
    import torch
    if tree_name == "small":
        select_kernel(monkeypatch, "paired")
        _, db = small_case
    else:
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        tree = synth.make_tree(LARGE[tree_name], seed=30)
        db = synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    rng = np.random.default_rng(21)
    reads = _reads(db.kmer_size, rng, 1500)
    weights = rng.integers(0, 1 << 32, size=len(reads), dtype=np.uint64).astype(np.uint32)
    num_samples = 7
    samples = _mixed_samples(len(reads), num_samples, rng)
    results = {}
    variants = [("one call", {}), ("uneven pieces", {}), ("two streams", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"}),
                ("global path", {"EPIK_AMD_PROFILE_LDS": "0"}), ("lds path", {"EPIK_AMD_PROFILE_LDS": "1"})]
    for name, env in variants:
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.cohort(num_samples) as cohort:
            pl.choose_counts(200)
            batch = DeviceBatch(pl, reads, weights)
            d_samples = device_samples(batch, samples)
            if name == "uneven pieces":
                cuts = [0, 1, 64, 65, 700, 701, 1499, len(reads)]
                for a, b in zip(cuts, cuts[1:]):
                    add_to(batch, cohort, d_samples, a, b - a)
                add_to(batch, cohort, d_samples, 5, 0)            # n == 0: nothing
            elif name == "two streams":
                other = torch.cuda.Stream()
                add_to(batch, cohort, d_samples, 0, 700)
                add_to(batch, cohort, d_samples, 700, None, other)
            else:
                add_to(batch, cohort, d_samples)
            results[name] = cohort.read()
            if name == "one call":
                want = numpy_cohort(*batch.host(), weights, samples, num_samples, db.num_branches)
            if "EPIK_AMD_PROFILE_LDS" in env:
                assert cohort.lds_path == (env["EPIK_AMD_PROFILE_LDS"] == "1")
        for key in env:
            monkeypatch.delenv(key)
    assert want[3] == int((samples >= num_samples).sum()) > 2
    for name, got in results.items():
        assert_cells(got, want, name)


def add_host(cohort, rows, n_rows, counts, weights, samples):
    """Rows in host memory through Cohort.add_device."""
    import torch
    dev = torch.device("cuda", cohort.device)
    arrays = (np.ascontiguousarray(rows, dtype=capi.PLACEMENT).view(np.float64).reshape(-1),) + tuple(
        np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).reshape(-1) for a in (n_rows, counts, samples, weights))
    d_rows, d_n, d_counts, d_samples, d_w = (torch.from_numpy(a).to(dev) for a in arrays)
    torch.cuda.synchronize(dev)
    cohort.add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_samples.data_ptr(), len(n_rows), d_w.data_ptr())
    torch.cuda.synchronize(dev)


@pytest.mark.parametrize("lds", ["1", "0"])
@pytest.mark.parametrize("keep", OTHER_KEEPS)
def test_cohort_at_other_keep_at_most(placer_cls, monkeypatch, keep, lds):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", lds)
    _, db = keep_case()
    rng = np.random.default_rng(100 + keep)
    reads = _reads(db.kmer_size, rng, 600)
    weights = rng.integers(0, 5, size=len(reads)).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    num_samples = 7
    with placer_cls.from_synth(db, keep_at_most=keep) as pl, pl.cohort(num_samples) as cohort:
        assert pl.keep_at_most == keep and cohort.lds_path == (lds == "1")
        # the rows the placement has just written
        pl.choose_counts(200)
        batch = DeviceBatch(pl, reads, weights)
        samples = _mixed_samples(len(reads), num_samples, rng)
        add_to(batch, cohort, device_samples(batch, samples))
        want = numpy_cohort(*batch.host(), weights, samples, num_samples, db.num_branches)
        assert_cells(cohort.read(), want, f"placed rows, keep {keep}")
        assert want[3] > 2 and sum(t["placed"] for t in want[2]) > 0 and sum(t["bad_rows"] for t in want[2]) == 0
        # forged rows: bad rows in the workgroup's current sample and in any other -- the current sample changes within
        # the batch, run by run and, interleaved, tile by tile --, reads of no sample, one sample without reads
        rows, n_rows, counts, weights = forged_rows(rng, 700, keep, db.num_branches)
        for name in ("runs", "interleaved"):
            samples = _mixed_samples(700, num_samples, rng) if name == "runs" else (np.arange(700) % (num_samples + 2)).astype(np.uint32)
            samples[samples == 3] = 1
            want = numpy_cohort(rows, n_rows, counts, weights, samples, num_samples, db.num_branches)
            cohort.reset()
            add_host(cohort, rows, n_rows, counts, weights, samples)
            assert_cells(cohort.read(), want, f"forged rows, {name}, keep {keep}")
            assert want[3] > 0 and not want[0][3].any() and sum(want[2][3].values()) == 0
            assert sum(1 for t in want[2] if t["bad_rows"] > 0) >= 2
            assert ((n_rows == keep + 5) & (counts[:, 0] != 0) & (samples < num_samples)).sum() > 0


def test_a_read_of_no_sample_adds_to_bad_samples_and_nothing_else(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    reads = _reads(db.kmer_size, np.random.default_rng(4))
    with placer_cls.from_synth(db) as pl, pl.cohort(3) as cohort:
        batch = DeviceBatch(pl, reads)
        for value in (3, 4, 0x7FFFFFFF, 0xFFFFFFFF):
            cohort.reset()
            add_to(batch, cohort, device_samples(batch, np.full(len(reads), value, dtype=np.uint32)))
            got = cohort.read()
            assert got.bad_samples == len(reads), value
            assert not got.mass.any() and not got.best.any() and not got.totals.view(U64).any(), value
        # one read of a sample among them: only its cells move
        samples = np.full(len(reads), 3, dtype=np.uint32)
        samples[100] = 2
        cohort.reset()
        add_to(batch, cohort, device_samples(batch, samples))
        assert_cells(cohort.read(), numpy_cohort(*batch.host(), None, samples, 3, db.num_branches))
        assert cohort.read().bad_samples == len(reads) - 1 and cohort.read().records()[2] == 1
        # a cohort without samples, and one of another placer's shape
        with pytest.raises(capi.EpikAmdError) as e:
            pl.cohort(0)
        assert e.value.code == capi.ERR_INVALID and "num_samples is 0" in str(e.value)
        data, offs = synth.pack_reads(reads)
        with placer_cls.from_synth(db, keep_at_most=3) as other, pytest.raises(capi.EpikAmdError) as e:
            other.cohort_packed(cohort, data, offs, np.zeros(len(reads), np.uint32))
        assert e.value.code == capi.ERR_INVALID and "another placer" in str(e.value)


def test_the_four_host_entries_equal_the_rule_over_the_placed_rows(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    _, db = small_case
    rng = np.random.default_rng(31)
    reads = _reads(db.kmer_size, rng, 329)              # 333 reads; pairs: 166
    reads = reads[:332]
    num_samples = 6
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.cohort(num_samples) as cohort:
        entries = (("reads", {}, "EPIK_AMD_PROFILE_CHUNK_READS", lambda: pl.place_packed(data, offs)),
                   ("strands", {"strand": "both"}, "EPIK_AMD_STRAND_CHUNK_READS", lambda: pl.place_strands(data, offs, "both")),
                   ("mates", {"mates": "fr", "strand": "both"}, "EPIK_AMD_MATES_CHUNK_READS",
                    lambda: pl.place_mates(data, offs, "both", "fr")))
        for name, kw, env, place in entries:
            placed = place()
            rows, n_rows, counts = placed[:3]
            n = len(n_rows)
            assert n == (166 if name == "mates" else 332)
            weights = rng.integers(0, 9, size=n).astype(np.uint32)
            samples = (np.arange(n) * num_samples // n).astype(np.uint32)       # grouped: chunks of five cut inside samples
            samples[7::50] = num_samples                                        # ... and some reads of no sample
            want = numpy_cohort(rows, n_rows, counts, weights, samples, num_samples, db.num_branches)
            for chunk in (None, "5"):
                if chunk:
                    monkeypatch.setenv(env, chunk)
                cohort.reset()
                labels = pl.cohort_packed(cohort, data, offs, samples, weights, **kw)
                monkeypatch.delenv(env, raising=False)
                assert_cells(cohort.read(), want, (name, chunk))
                assert (labels is None) if len(placed) == 3 else np.array_equal(labels, placed[3])
        with pytest.raises(ValueError):
            pl.cohort_packed(cohort, data, offs, np.zeros(5, np.uint32))
        with pytest.raises(capi.EpikAmdError) as e:             # frames need an amino-acid handle
            pl.cohort_packed(cohort, data, offs, np.zeros(332, np.uint32), translate="both")
        assert e.value.code == capi.ERR_UNSUPPORTED


def test_cohort_frames_equal_the_rule_over_the_placed_rows(placer_cls, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT" if i % 3 else "ACGTUNRYKMSWBDHV-."), size=int(rng.integers(0, 200)))) for i in range(300)]
    reads += ["", "AC", "TAATAGTGATAATAGTGA", "NNNNNNNNNNNN"]
    weights = rng.integers(0, 9, size=len(reads)).astype(np.uint32)
    samples = (np.arange(len(reads)) * 4 // len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.cohort(4) as cohort:
        rows, n_rows, counts, frames = pl.place_frames(data, offs, "both")
        want = numpy_cohort(rows, n_rows, counts, weights, samples, 4, db.num_branches)
        assert sum(t["placed"] for t in want[2]) > 0 and sum(t["too_short"] for t in want[2]) > 0
        for chunk in (None, "5"):
            if chunk:
                monkeypatch.setenv("EPIK_AMD_FRAME_CHUNK_READS", chunk)
            cohort.reset()
            got_frames = pl.cohort_packed(cohort, data, offs, samples, weights, translate="both")
            monkeypatch.delenv("EPIK_AMD_FRAME_CHUNK_READS", raising=False)
            assert_cells(cohort.read(), want, f"frames, chunk {chunk}")
            assert np.array_equal(got_frames, frames)


# ---- the KR kernel ---------------------------------------------------------------------------------------------------
KR_TREES = {7: 4, 999: 500, 5199: 2600}
KR_CASES = {}


def kr_case(num_branches):
    """(parent, branch_length, first, db) of a tree of that many branches; 10 399: the ladder.  Some lengths are 0."""
    if num_branches not in KR_CASES:
        if num_branches == 10_399:
            parent, bl = caterpillar(10_399)
        else:
            tree = synth.make_tree(KR_TREES[num_branches], seed=30)
            parent, bl = tree.parent, tree.branch_length
        bl = np.array(bl, dtype=np.float64)
        bl[::5] = 0.0
        parent = np.asarray(parent, dtype=np.int64)
        assert len(parent) == num_branches
        db = synth.make_db(num_branches, kmer_size=4, seed=31, p_present=0.7)
        KR_CASES[num_branches] = (parent, bl, numpy_first(parent), db)
    return KR_CASES[num_branches]


@pytest.mark.parametrize("num_branches", [7, 999, 5199, 10_399])
def test_kr_equals_the_host_mirror_and_the_restatement_bit_for_bit(placer_cls, monkeypatch, num_branches):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(num_branches)
    rng = np.random.default_rng(num_branches)
    with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree:
        for num_samples in (1, 2, 33, 70):
            mass = random_cells(rng, num_samples, num_branches, empty=1)
            want = numpy_kr(mass, first, bl)
            assert same_bits(cohort_mod.kr_host(mass, first, bl), want)
            with pl.cohort(num_samples) as cohort:
                best = rng.integers(0, 1 << 40, size=mass.shape, dtype=np.uint64)
                cohort.add_cells(mass // U64(2), best, None)
                cohort.add_cells(mass - mass // U64(2), None, None)              # in two halves: add_cells adds
                back = cohort.read()
                assert np.array_equal(back.mass, mass) and np.array_equal(back.best, best) and not back.totals.view(U64).any()
                got = cohort.kr(tree, bl)
                assert same_bits(got, want), (num_samples, np.argwhere(got.view(U64) != want.view(U64))[:10])
                # into a poisoned buffer on a stream of its own: every cell written, the same bits; and a second time
                d_out = torch.full((num_samples * num_samples,), float("nan"), dtype=torch.float64, device=f"cuda:{pl.device}")
                stream = torch.cuda.Stream()
                torch.cuda.synchronize()
                cohort.kr_device(tree, bl, d_out.data_ptr(), stream.cuda_stream)
                stream.synchronize()
                assert same_bits(d_out.cpu().numpy().reshape(num_samples, num_samples), want), num_samples
                if num_samples > 1:
                    assert (got[1] == np.where(np.arange(num_samples) == 1, 0.0, -1.0)).all()


def test_kr_of_a_placed_cohort_and_under_two_workgroups(placer_cls, monkeypatch):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    parent, bl, first, db = kr_case(999)
    reads = _reads(db.kmer_size, np.random.default_rng(9))
    num_samples = 33
    samples = (np.arange(len(reads)) * (num_samples - 1) // len(reads)).astype(np.uint32)
    samples = np.where(samples >= 4, samples + 1, samples).astype(np.uint32)        # sample 4 stays empty
    data, offs = synth.pack_reads(reads)
    results = {}
    for name, env in (("default", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(parent, bl) as tree, pl.cohort(num_samples) as cohort:
            pl.cohort_packed(cohort, data, offs, samples)
            cells = cohort.read()
            results[name] = (cells, cohort.kr(tree, bl))
            # errors of kr: another tree, a bad length
            from epik_amd.confidence import Tree
            with Tree(pl.device, *kr_case(7)[:2]) as small_tree, pytest.raises(capi.EpikAmdError) as e:
                cohort.kr(small_tree, bl)
            assert e.value.code == capi.ERR_INVALID and "tree" in str(e.value)
            bad = bl.copy()
            bad[17] = -1.0
            with pytest.raises(capi.EpikAmdError) as e:
                cohort.kr(tree, bad)
            assert e.value.code == capi.ERR_INVALID and "branch 17" in str(e.value)
        for key in env:
            monkeypatch.delenv(key)
    cells, kr = results["default"]
    assert cells.mass.any(axis=1).sum() >= 30 and not cells.mass[4].any()
    want = numpy_kr(cells.mass, first, bl)
    assert same_bits(kr, want) and same_bits(kr, cohort_mod.kr_host(cells.mass, first, bl))
    assert (kr[4] == np.where(np.arange(num_samples) == 4, 0.0, -1.0)).all()
    assert np.array_equal(results["two workgroups"][0].mass, cells.mass) and same_bits(results["two workgroups"][1], kr)


# ---- the drivers, end to end -----------------------------------------------------------------------------------------
def _run(argv):
    run = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, " ".join(argv) + run.stdout[-2000:] + run.stderr[-2000:]
    return run


def _cohort_files(path, list_name="samples.list"):
    return {what: (path / f"cohort_{what}_{list_name}.tsv") for what in ("samples", "profile", "kr")}


def _check_driver(tmp_path, binary, db_path, tree, sample_reads, flags, variants):
    """`binary --cohort` over the samples under every variant of the command line: the same bytes; every sample's cells
    those of --profile-only on that sample alone; the KR file the bits of kr_host on the profile file's masses."""
    driver = os.path.join(ROOT, "epik_amd", "bin", binary)
    names = list(sample_reads)
    lines = ["# name<TAB>path", ""]
    for i, (name, reads) in enumerate(sample_reads.items()):
        folder = tmp_path / ("in" if i % 2 else "in/deeper")
        folder.mkdir(parents=True, exist_ok=True)
        _write_fasta(str(folder / f"{name}.fasta"), [(f"{name}_{j}", s) for j, s in enumerate(reads)])
        lines.append(f"{name}\t{folder.relative_to(tmp_path)}/{name}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant)
        outs[variant].mkdir()
        _run([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"] + flags + extra)
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(p.name for p in _cohort_files(outs[variant]).values())
    first_variant = next(iter(variants))
    files = _cohort_files(outs[first_variant])
    for variant in variants:
        for what, path in _cohort_files(outs[variant]).items():
            assert path.read_bytes() == files[what].read_bytes(), (variant, what)
    n = tree.num_nodes
    got_names, totals = cohort_mod.read_samples_tsv(str(files["samples"]))
    assert got_names == names
    mass, best = cohort_mod.read_profile_tsv(str(files["profile"]), names, n)
    for s, name in enumerate(names):
        alone = tmp_path / ("alone_" + name)
        alone.mkdir()
        fasta = next(tmp_path.glob(f"in/**/{name}.fasta"))
        _run([driver, "-d", db_path, "-q", str(fasta), "-o", str(alone), "--profile-only"] + flags)
        back = profile_mod.read_tsv(str(alone / f"profile_{name}.fasta.tsv"))
        assert np.array_equal(back["mass_q"], mass[s]) and np.array_equal(back["best"], best[s]), name
        for k in ("records", "placed", "no_hit", "too_short"):
            assert int(totals[k][s]) == back[k], (name, k)
        assert int(totals["too_narrow"][s]) == 0 and int(totals["total_mass_q"][s]) == int(mass[s].sum(dtype=U64))
    kr_names, kr = cohort_mod.read_kr_tsv(str(files["kr"]))
    assert kr_names == names
    want = cohort_mod.kr_host(mass, numpy_first(tree.parent), tree.branch_length)
    assert same_bits(kr, want), (kr, want)
    return totals, kr


def test_epik_dna_cohort_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(60, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=30, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    sizes = {"gut_1": 300, "gut_2": 120, "soil": 40, "blank": 45, "skin 3": 210}
    samples = {}
    for i, (name, size) in enumerate(sizes.items()):
        if name == "blank":                               # no placeable read: too short, or no k-mer of the database
            samples[name] = ["ACG", "AC", "A"] * 15
            continue
        data, offs = synth.make_clade_reads(refs[i * 5:i * 5 + 8], size, 150, seed=20 + i)
        reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        samples[name] = reads + reads[:size // 10] + ["ACG"]      # duplicated records, a too short one
    variants = {"j1": ["-j", "1"], "j16": ["-j", "16"], "two_handles": ["--devices", "0,0", "-j", "4"],
                "batch50": ["--batch-size", "50"]}
    totals, kr = _check_driver(tmp_path, "epik-dna", db_path, tree, samples, [], variants)
    assert int(totals["placed"][3]) == 0 and int(totals["records"][3]) == 45 and (np.delete(totals["placed"], 3) > 0).all()
    assert (kr[3] == np.where(np.arange(5) == 3, 0.0, -1.0)).all() and (np.delete(np.delete(kr, 3, 0), 3, 1)[~np.eye(4, dtype=bool)] > 0).all()
    # both strands: the reads of one sample reversed
    from test_strand_gpu import rc
    samples["soil"] = [rc(r) for r in samples["soil"]]
    both = tmp_path / "both"
    both.mkdir()
    totals_both, kr_both = _check_driver(both, "epik-dna", db_path, tree, samples, ["--strand", "both"], {"j4": ["-j", "4"]})
    assert np.array_equal(totals_both["records"], totals["records"]) and int(totals_both["placed"][2]) > 0
    # the launcher passes the flag on
    import sys
    out_l = tmp_path / "launcher"
    out_l.mkdir()
    _run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(out_l), "--cohort",
          str(tmp_path / "samples.list")])
    assert (out_l / "cohort_kr_samples.list.tsv").read_bytes() == (tmp_path / "out_j1" / "cohort_kr_samples.list.tsv").read_bytes()


def test_epik_aa_cohort_with_translated_reads(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    db_path = str(tmp_path / "aa.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    rng = np.random.default_rng(41)
    samples = {}
    for name, size in (("a", 120), ("b", 40), ("none", 50), ("c", 300), ("d", 77)):
        if name == "none":
            samples[name] = ["AC", "ACGTA", "T"] * 16 + ["A", "C"]
        else:
            samples[name] = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(30, 200)))) for _ in range(size)]
    totals, kr = _check_driver(tmp_path, "epik-aa", db_path, tree, samples, ["--translate", "both"],
                               {"j1": ["-j", "1"], "batch50_two_handles": ["--batch-size", "50", "--devices", "0,0"]})
    assert int(totals["placed"][2]) == 0 and (np.delete(totals["placed"], 2) > 0).all() and (kr[2, [0, 1, 3, 4]] == -1.0).all()
