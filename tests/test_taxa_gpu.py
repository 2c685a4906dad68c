"""Taxonomic assignment on the GPU (epik_amd_taxonomy_*, taxa_place.hip): the records and the cells of add_device against
the numpy rule bit for bit on the forged batches of test_taxa_cpu -- every lane-group width 1 to 64, every tau_q, 1, 3
and 64 samples grouped and interleaved, weights 0 and 2^32 - 1, one workgroup, the LDS and the global path, taxonomies
of the one-workgroup-a-CU regime and beyond the LDS limit, two calls on two streams --, cells without records, and the
rows a real placement wrote, where the cells also meet the profile of the same rows."""
import numpy as np
import pytest

from conftest import select_kernel
from epik_amd import capi, synth, taxonomy
from test_profile_gpu import DeviceBatch, _reads
from test_taxa_cpu import FORGED_KEEPS, FORGED_N, FORGED_TAUS, SHAPES, forged, same_bits

pytestmark = pytest.mark.gpu
U64 = np.uint64
ENV = ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT", "EPIK_AMD_PROFILE_LDS")
READS = 2048                                       # of the 4 096 forged reads: the strides of the forging are far shorter
POISON = 0x5A5A5A5A


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


@pytest.fixture(scope="module")
def forged_db():
    return synth.make_db(FORGED_N, kmer_size=4, seed=31, p_present=0.7)


def chain_and_star(num_taxa):
    """taxon_parent of half a star under the root and a chain of the other half: (parent with -1 for the root)."""
    leaves = num_taxa // 2
    parent = np.full(num_taxa, num_taxa - 1, np.int64)
    parent[leaves:num_taxa - 1] = np.arange(leaves + 1, num_taxa)
    parent[-1] = -1
    return parent


class DeviceRows:
    """Host rows uploaded once, a record buffer with a poisoned region behind it."""

    def __init__(self, device, rows, n_rows, counts):
        import torch
        self.torch, self.n, self.keep = torch, len(n_rows), rows.shape[1]
        self.dev = torch.device("cuda", device)
        up = lambda a: torch.from_numpy(a).to(self.dev)
        self.d_rows = up(np.ascontiguousarray(rows, dtype=capi.PLACEMENT).view(np.float64).reshape(-1))
        self.d_n = up(np.ascontiguousarray(n_rows, dtype=np.uint32).view(np.int32))
        self.d_counts = up(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32).reshape(-1))
        self.d_records = torch.full((self.n * 4 + 1024,), POISON, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)

    def u32(self, a):
        return None if a is None else self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(self.dev)

    def add(self, tx, tau_q, d_weights=None, d_samples=None, first=0, count=None, stream=None, records=True):
        count = self.n - first if count is None else count
        ptr = lambda t, size: 0 if t is None else t.data_ptr() + first * size
        tx.add_device(self.d_rows.data_ptr() + first * self.keep * 16, self.d_n.data_ptr() + first * 4,
                      self.d_counts.data_ptr() + first * self.keep * 4, count, tau_q,
                      self.d_records.data_ptr() + first * 16 if records else 0, ptr(d_weights, 4), ptr(d_samples, 4),
                      0 if stream is None else stream.cuda_stream)

    def records(self):
        """The records, after the poisoned region has been seen untouched; the buffer is poisoned again."""
        self.torch.cuda.synchronize(self.dev)
        raw = self.d_records.cpu().numpy().view(np.uint32)
        assert (raw[self.n * 4:] == POISON).all(), "the kernel wrote behind the records"
        self.d_records.fill_(POISON)
        return raw[:self.n * 4].copy().view(capi.TAXON_RECORD)


def sample_layouts(n, num_samples, rng):
    """Weights with 0 and 2^32 - 1; samples grouped (one of them empty, a few reads of no sample) and interleaved."""
    weights = rng.integers(0, 5, size=n).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    grouped = (np.arange(n, dtype=np.int64) * num_samples // n).astype(np.uint32)
    if num_samples > 2:
        grouped[grouped == num_samples // 2] = num_samples // 2 - 1
    grouped[3::97] = num_samples + 5
    grouped[n - 1] = 0xFFFFFFFF
    interleaved = (np.arange(n) % (num_samples + 1)).astype(np.uint32)       # (one in S + 1 of no sample)
    return weights, {"grouped": grouped, "interleaved": interleaved}


def assert_cells(got, want, what):
    assert np.array_equal(got.totals, want.totals), (what, got.totals, want.totals)
    assert got.bad_samples == want.bad_samples, (what, got.bad_samples, want.bad_samples)
    assert np.array_equal(got.assigned, want.assigned), (what, np.argwhere(got.assigned != want.assigned)[:10])
    assert np.array_equal(got.direct, want.direct), (what, np.argwhere(got.direct != want.direct)[:10])


# (one workgroup walks every tile: its LDS cells are carried from tile to tile, flushed and zeroed again where the next
# tile begins in another sample, and interleaved reads split into the current sample's and the others')
VARIANTS = [("as created", {}), ("one workgroup, global", {"EPIK_AMD_MAX_BLOCKS": "1", "EPIK_AMD_PROFILE_LDS": "0"}),
            ("one workgroup, lds", {"EPIK_AMD_MAX_BLOCKS": "1", "EPIK_AMD_PROFILE_LDS": "1"}), ("lds", {"EPIK_AMD_PROFILE_LDS": "1"})]


@pytest.mark.parametrize("keep", FORGED_KEEPS)
def test_kernel_equals_numpy_bit_for_bit_on_forged_rows(placer_cls, forged_db, monkeypatch, keep):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    rows, n_rows, counts = (a[:READS] for a in forged(keep))
    rng = np.random.default_rng(keep)
    layouts = {S: sample_layouts(READS, S, rng) for S in (1, 3, 64)}
    wanted = {}
    for name, (taxon_parent, label) in SHAPES.items():
        for tq in FORGED_TAUS:
            wanted[name, tq] = taxonomy.numpy_records(taxon_parent, label, rows, n_rows, counts, tq)
    launches = 0
    for variant, env in VARIANTS:
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(forged_db, keep_at_most=keep) as pl:
            dev = DeviceRows(pl.device, rows, n_rows, counts)
            for name, (taxon_parent, label) in SHAPES.items():
                for S, (weights, samples_of) in layouts.items():
                    d_w = dev.u32(weights)
                    with pl.taxonomy(taxon_parent, label, S) as tx:
                        assert tx.lds_path == (env.get("EPIK_AMD_PROFILE_LDS") != "0")
                        for tq in FORGED_TAUS:
                            want, state = wanted[name, tq]
                            for layout, samples in samples_of.items():
                                tx.reset()
                                dev.add(tx, tq, d_w, dev.u32(samples))
                                what = (variant, name, S, tq, layout)
                                got = dev.records()
                                assert same_bits(got, want), (what, np.nonzero(got != want)[0][:10])
                                assert_cells(tx.read(), taxonomy.numpy_cells(state, weights, samples, S), what)
                                launches += 1
        for key in env:
            monkeypatch.delenv(key)
    assert launches == len(VARIANTS) * len(SHAPES) * 3 * len(FORGED_TAUS) * 2


@pytest.mark.parametrize("num_taxa,lds", [(5000, True), (12000, False)])
def test_taxonomies_of_a_workgroup_a_cu_and_beyond_the_lds_limit(placer_cls, forged_db, monkeypatch, num_taxa, lds):
    """16 * T bytes beside the kernel's own: T = 5 000 leaves a CU to one workgroup, T = 12 000 goes to global memory."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    keep = 7
    rows, n_rows, counts = (a[:READS] for a in forged(keep))
    rng = np.random.default_rng(num_taxa)
    taxon_parent = chain_and_star(num_taxa)
    label = rng.integers(0, num_taxa, size=FORGED_N).astype(np.uint32)
    label[::3] = rng.integers(num_taxa // 2, num_taxa, size=len(label[::3]))       # many on the chain: nested clades
    S = 3
    weights, samples_of = sample_layouts(READS, S, rng)
    tq = FORGED_TAUS[1]
    want, state = taxonomy.numpy_records(taxon_parent, label, rows, n_rows, counts, tq)
    assert len(set(want["taxon"][want["taxon"] < num_taxa].tolist())) > 50
    for blocks in (None, "1"):                     # as created; one workgroup for all the tiles, in its path as created
        if blocks:
            monkeypatch.setenv("EPIK_AMD_MAX_BLOCKS", blocks)
        with placer_cls.from_synth(forged_db, keep_at_most=keep) as pl, pl.taxonomy(taxon_parent, label, S) as tx:
            assert tx.lds_path == lds
            dev = DeviceRows(pl.device, rows, n_rows, counts)
            d_w = dev.u32(weights)
            for layout, samples in samples_of.items():
                tx.reset()
                dev.add(tx, tq, d_w, dev.u32(samples))
                got = dev.records()
                assert same_bits(got, want), (blocks, layout, np.nonzero(got != want)[0][:10])
                assert_cells(tx.read(), taxonomy.numpy_cells(state, weights, samples, S), (num_taxa, blocks, layout))
    monkeypatch.delenv("EPIK_AMD_MAX_BLOCKS")
    with placer_cls.from_synth(forged_db, keep_at_most=keep) as pl:
        if not lds:
            monkeypatch.setenv("EPIK_AMD_PROFILE_LDS", "1")
            with pytest.raises(capi.EpikAmdError) as e:
                pl.taxonomy(taxon_parent, label, S)
            assert e.value.code == capi.ERR_UNSUPPORTED


def test_two_streams_no_records_add_cells_and_refusals(placer_cls, forged_db, monkeypatch):
    import torch
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    keep, S = 13, 3
    rows, n_rows, counts = (a[:READS] for a in forged(keep))
    taxon_parent, label = SHAPES["synth"]
    weights, samples_of = sample_layouts(READS, S, np.random.default_rng(5))
    samples = samples_of["grouped"]
    tq = FORGED_TAUS[1]
    want, state = taxonomy.numpy_records(taxon_parent, label, rows, n_rows, counts, tq)
    cells = taxonomy.numpy_cells(state, weights, samples, S)
    with placer_cls.from_synth(forged_db, keep_at_most=keep) as pl, pl.taxonomy(taxon_parent, label, S) as tx:
        dev = DeviceRows(pl.device, rows, n_rows, counts)
        d_w, d_s = dev.u32(weights), dev.u32(samples)
        # two calls on two streams: the cells of one call, and every record
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        dev.add(tx, tq, d_w, d_s, 0, 777, a)
        dev.add(tx, tq, d_w, d_s, 777, None, b)
        dev.add(tx, tq, d_w, d_s, 5, 0, b)                   # n == 0: nothing
        assert same_bits(dev.records(), want)
        assert_cells(tx.read(), cells, "two streams")
        # no records: the same cells, and nothing is written anywhere near the buffer
        tx.reset()
        dev.add(tx, tq, d_w, d_s, records=False)
        assert_cells(tx.read(), cells, "cells only")
        torch.cuda.synchronize()
        assert (dev.d_records.cpu().numpy().view(np.uint32) == POISON).all()
        # no weights, no samples: every read once into row 0
        tx.reset()
        dev.add(tx, tq)
        assert_cells(tx.read(), taxonomy.numpy_cells(state, None, None, S), "no weights, no samples")
        # add_cells: what another device's object read, summed in; wrapping
        tx.add_cells(cells)
        twice = tx.read()
        assert np.array_equal(twice.direct, taxonomy.numpy_cells(state, None, None, S).direct + cells.direct)
        assert np.array_equal(twice.totals["placed"], taxonomy.numpy_cells(state, None, None, S).totals["placed"] + cells.totals["placed"])
        # refusals, each with its cause
        for bad_tau in (0, 1 << 29, (1 << 30) + 1):
            with pytest.raises(capi.EpikAmdError) as e:
                dev.add(tx, bad_tau)
            assert e.value.code == capi.ERR_INVALID and "tau_q" in str(e.value)
        with pytest.raises(capi.EpikAmdError) as e:
            tx.add_device(0, dev.d_n.data_ptr(), dev.d_counts.data_ptr(), 4, tq)
        assert e.value.code == capi.ERR_INVALID and "null device buffer" in str(e.value)
        with pytest.raises(capi.EpikAmdError) as e:
            pl.taxonomy(taxon_parent, label, 0)
        assert "num_samples is 0" in str(e.value)
        bad_label = label.copy()
        bad_label[17] = len(taxon_parent)
        with pytest.raises(capi.EpikAmdError) as e:
            pl.taxonomy(taxon_parent, bad_label, 1)
        assert e.value.code == capi.ERR_INVALID and "branch 17:" in str(e.value)
        bad_parent = np.array(taxon_parent).copy()
        bad_parent[4] = 2
        with pytest.raises(capi.EpikAmdError) as e:
            pl.taxonomy(bad_parent, label, 1)
        assert e.value.code == capi.ERR_INVALID and "taxon 4:" in str(e.value) and "branch" not in str(e.value)


def test_placed_rows_meet_numpy_and_the_profile(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    tree, db = small_case
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, 3, seed=8))
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    assert taxa.num_taxa > 4 and len(set(label.tolist())) > 4 and (label == taxa.num_taxa - 1).any()
    rng = np.random.default_rng(11)
    reads = _reads(db.kmer_size, rng)
    weights = rng.integers(0, 5, size=len(reads)).astype(np.uint32)
    tq = taxonomy.mass_tau_q(0.95)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile, pl.taxonomy(taxa.parent, label) as tx:
        assert pl.keep_at_most == 7
        batch = DeviceBatch(pl, reads, weights)
        d_records = batch.torch.full((batch.n * 4,), POISON, dtype=batch.torch.int32, device=batch.d_n.device)
        tx.add_device(batch.d_rows.data_ptr(), batch.d_n.data_ptr(), batch.d_counts.data_ptr(), batch.n, tq,
                      d_records.data_ptr(), batch.d_w.data_ptr(), 0, batch.stream.cuda_stream)
        batch.add_to(profile)
        batch.stream.synchronize()
        got_cells, whole = tx.read(), profile.read()
        got = d_records.cpu().numpy().view(np.uint32).view(capi.TAXON_RECORD)
        rows, n_rows, counts = batch.host()
    want, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq, weights)
    assert same_bits(got, want), np.nonzero(got != want)[0][:10]
    assert_cells(got_cells, cells, "placed rows")
    placed = want["taxon"] < taxa.num_taxa
    assert placed.sum() > 300 and (want["taxon"] == capi.TAXON_NO_HIT).sum() > 0 and (want["taxon"] == capi.TAXON_TOO_SHORT).sum() > 0
    assert (want["taxon"][placed] != want["first_taxon"][placed]).sum() > 20            # not simply the best row's taxon
    # (the profile knows no NO_MASS: such a read is placed there, and adds no mass in either)
    assert int(got_cells.assigned.sum(dtype=U64)) == int(got_cells.totals["placed"][0])
    assert int(got_cells.totals["placed"][0] + got_cells.totals["no_mass"][0]) == whole.totals["placed"]
    by_label = np.zeros(taxa.num_taxa, U64)
    np.add.at(by_label, label.astype(np.int64), whole.mass)
    assert np.array_equal(got_cells.direct[0], by_label)


def _host_entry_case(pl, taxa, label, data, offs, name, kw, env, place, rng, monkeypatch):
    """One host entry against its place_* twin followed by the rule on the host: with a chained profile, with a chained
    cohort, with every output pointer NULL, in one chunk and in chunks of five."""
    from test_cohort_cpu import assert_cells as assert_cohort_cells, numpy_cohort
    from test_profile_gpu import assert_profile, numpy_rule
    S, tq = 4, taxonomy.mass_tau_q(0.95)
    placed = place()
    rows, n_rows, counts = placed[:3]
    n = len(n_rows)
    weights = rng.integers(0, 9, size=n).astype(np.uint32)
    samples = (np.arange(n) * S // n).astype(np.uint32)             # grouped: chunks of five cut inside samples
    samples[7::50] = S                                              # ... and some reads of no sample
    want, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq, weights, samples, S)
    assert (want["taxon"] < taxa.num_taxa).sum() > n // 3
    with pl.taxonomy(taxa.parent, label, S) as tx, pl.profile() as profile, pl.cohort(S) as cohort:
        for chunk in (None, "5"):
            if chunk:
                monkeypatch.setenv(env, chunk)
            # the twin's outputs and the records; a chained profile
            tx.reset(), profile.reset()
            got = pl.taxa_packed(tx, data, offs, tq, weights, samples, profile=profile, **kw)
            for a, b in zip(got[:3], placed[:3]):
                assert same_bits(a, b), (name, chunk)
            assert (got[3] is None) if len(placed) == 3 else np.array_equal(got[3], placed[3])
            assert same_bits(got[4], want), (name, chunk, np.nonzero(got[4] != want)[0][:10])
            assert_cells(tx.read(), cells, (name, chunk, "profile"))
            assert_profile(profile.read(), numpy_rule(rows, n_rows, counts, weights, db_branches(pl)), (name, chunk))
            # a chained cohort, and every output pointer NULL: cells only
            tx.reset(), cohort.reset()
            got = pl.taxa_packed(tx, data, offs, tq, weights, samples, cohort=cohort, rows_out=False, records_out=False, **kw)
            assert got[0] is None and got[1] is None and got[2] is None and got[4] is None
            assert_cells(tx.read(), cells, (name, chunk, "cohort, cells only"))
            assert_cohort_cells(cohort.read(), numpy_cohort(rows, n_rows, counts, weights, samples, S, db_branches(pl)), (name, chunk))
            monkeypatch.delenv(env, raising=False)
        # no weights and no samples: every item once, into row 0
        tx.reset()
        pl.taxa_packed(tx, data, offs, tq, rows_out=False, records_out=False, **kw)
        assert_cells(tx.read(), taxonomy.numpy_cells(taxonomy.numpy_records(taxa.parent, label, rows, n_rows, counts, tq)[1], None, None, S), name)
        return tx_refusals(pl, tx, profile, cohort, data, offs, n, tq, kw) if name == "reads" else None


def db_branches(pl):
    return pl.num_branches


def tx_refusals(pl, tx, profile, cohort, data, offs, n, tq, kw):
    for bad_tau in (0, 1 << 29, (1 << 30) + 1):
        with pytest.raises(capi.EpikAmdError) as e:
            pl.taxa_packed(tx, data, offs, bad_tau)
        assert e.value.code == capi.ERR_INVALID and "tau_q" in str(e.value)
    with pytest.raises(capi.EpikAmdError) as e:
        pl.taxa_packed(tx, data, offs, tq, profile=profile, cohort=cohort, samples=np.zeros(n, np.uint32))
    assert e.value.code == capi.ERR_INVALID and "not both" in str(e.value)
    with pytest.raises(capi.EpikAmdError) as e:
        pl.taxa_packed(tx, data, offs, tq, cohort=cohort)
    assert e.value.code == capi.ERR_INVALID and "samples" in str(e.value)
    with pytest.raises(ValueError):
        pl.taxa_packed(tx, data, offs, tq, weights=np.zeros(5, np.uint32))


def test_the_host_entries_equal_their_twins_and_the_rule(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    tree, db = small_case
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, 3, seed=8))
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    rng = np.random.default_rng(31)
    reads = _reads(db.kmer_size, rng, 329)[:332]                    # pairs: 166
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl:
        entries = (("reads", {}, "EPIK_AMD_CONFIDENCE_CHUNK_READS", lambda: pl.place_packed(data, offs)),
                   ("strands", {"strand": "both"}, "EPIK_AMD_STRAND_CHUNK_READS", lambda: pl.place_strands(data, offs, "both")),
                   ("mates", {"mates": "fr", "strand": "both"}, "EPIK_AMD_MATES_CHUNK_READS",
                    lambda: pl.place_mates(data, offs, "both", "fr")))
        for name, kw, env, place in entries:
            _host_entry_case(pl, taxa, label, data, offs, name, kw, env, place, rng, monkeypatch)
        # an object of another placer's shape is refused, and frames need an amino-acid handle
        with placer_cls.from_synth(db, keep_at_most=3) as other, other.taxonomy(taxa.parent, label) as foreign:
            with pytest.raises(capi.EpikAmdError) as e:
                pl.taxa_packed(foreign, data, offs, 1 << 30)
            assert e.value.code == capi.ERR_INVALID and "another placer" in str(e.value)
        with pl.taxonomy(taxa.parent, label) as tx, pytest.raises(capi.EpikAmdError) as e:
            pl.taxa_packed(tx, data, offs, 1 << 30, translate="both")
        assert e.value.code == capi.ERR_UNSUPPORTED


def test_taxa_frames_equal_their_twin_and_the_rule(placer_cls, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, 3, seed=9))
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT" if i % 3 else "ACGTUNRYKMSWBDHV-."), size=int(rng.integers(0, 200)))) for i in range(300)]
    reads += ["", "AC", "TAATAGTGATAATAGTGA", "NNNNNNNNNNNN"]
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl:
        _host_entry_case(pl, taxa, label, data, offs, "frames", {"translate": "both"}, "EPIK_AMD_FRAME_CHUNK_READS",
                         lambda: pl.place_frames(data, offs, "both"), rng, monkeypatch)


# ---- the drivers, end to end -----------------------------------------------------------------------------------------
def _drive(argv):
    import subprocess
    run = subprocess.run(argv, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, " ".join(argv) + run.stdout[-2000:] + run.stderr[-2000:]


def _without_invocation(path):
    lines = path.read_bytes().split(b"\n")
    quoted = [i for i, line in enumerate(lines) if b'"invocation"' in line]
    assert len(quoted) == 1
    del lines[quoted[0]]
    return lines


def test_drivers_write_the_three_files(placer_cls, tmp_path):
    """About 2 000 reads in 3 samples on N = 199.  The files are the same bytes whatever -j, --batch-size and the devices,
    and equal the Python mirror's over the rows the library places (the oracle's LWRs differ from the device's by up to
    the parity bar of 1e-5, so its integer masses are not the same bits: the mirror starts from the library's rows, as
    the assign files' test does); everything else a run writes is what it is without --taxonomy."""
    import os
    import subprocess
    import sys
    from epik_amd import dbfile
    from test_profile_gpu import _write_fasta
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(100, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=40, ref_length=500, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    text = synth.synth_taxonomy(tree, 4, seed=14)
    (tmp_path / "taxonomy.tsv").write_text(text)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    tq = taxonomy.mass_tau_q(0.95)
    samples, lines = {}, []
    (tmp_path / "in").mkdir()
    for i, (name, size) in enumerate((("gut", 900), ("soil", 650), ("skin 3", 400))):
        data, offs = synth.make_clade_reads(refs[i * 10:i * 10 + 15], size, 150, seed=20 + i)
        reads = [bytes(data[int(offs[j]):int(offs[j + 1])]).decode() for j in range(size)]
        reads += reads[:size // 10] + ["ACG", "ACGTTGCAAC"]              # duplicated records, a too short one, a short one
        samples[name] = [(f"{name}_{j}", s) for j, s in enumerate(reads)]
        _write_fasta(str(tmp_path / "in" / f"{name}.fasta"), samples[name])
        lines.append(f"{name}\tin/{name}.fasta")
    (tmp_path / "samples.list").write_text("\n".join(lines) + "\n")
    # the mirror: every record once, in list order
    records = [r for name in samples for r in samples[name]]
    of_sample = np.concatenate([np.full(len(samples[name]), s, np.uint32) for s, name in enumerate(samples)])
    with placer_cls.from_synth(db, tree) as pl:
        rows, n_rows, counts = pl.place_packed(*synth.pack_reads([s for _, s in records]))
    want_records, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq, None, of_sample, 3)
    want_cohort = taxonomy.format_cohort_taxa_tsv(list(samples), cells, taxa, tq).encode()
    want_reads = taxonomy.format_taxa_reads_tsv([n for n, _ in records], want_records, taxa, tq).encode()
    placed = want_records["taxon"] < taxa.num_taxa
    assert placed.sum() > 1800 and (want_records["taxon"] == capi.TAXON_TOO_SHORT).sum() == 3 and len(records) > 2000
    assert len(set(want_records["taxon"][placed].tolist())) > 5
    driver = os.path.join(root, "epik_amd", "bin", "epik-dna")
    flags = ["--taxonomy", str(tmp_path / "taxonomy.tsv"), "--taxonomy-per-read"]
    cohort_taxa, taxa_reads = "cohort_taxa_samples.list.tsv", "taxa_reads_samples.list.tsv"
    variants = {"j1": ["-j", "1"], "j16": ["-j", "16"], "batch50": ["--batch-size", "50"], "batch777": ["--batch-size", "777"],
                "two_handles": ["--devices", "0,0", "-j", "4"], "without": None}
    outs = {}
    for variant, extra in variants.items():
        outs[variant] = tmp_path / ("out_" + variant)
        outs[variant].mkdir()
        _drive([driver, "-d", db_path, "-q", str(tmp_path / "samples.list"), "-o", str(outs[variant]), "--cohort"]
               + (flags + extra if extra is not None else []))
    others = sorted(p.name for p in outs["without"].iterdir())
    assert len(others) == 3
    for variant in variants:
        if variant == "without":
            continue
        assert sorted(p.name for p in outs[variant].iterdir()) == sorted(others + [cohort_taxa, taxa_reads]), variant
        assert (outs[variant] / cohort_taxa).read_bytes() == want_cohort, variant
        assert (outs[variant] / taxa_reads).read_bytes() == want_reads, variant
        for name in others:                                              # the cohort's own files are unchanged by the flag
            assert (outs[variant] / name).read_bytes() == (outs["without"] / name).read_bytes(), (variant, name)
    # one sample by itself: the jplace and the profile are what they are without the flag; the records never leave the
    # device without --taxonomy-per-read
    fasta = str(tmp_path / "in" / "gut.fasta")
    n_gut = len(samples["gut"])
    _, gut_cells = taxonomy.numpy_assign(taxa.parent, label, rows[:n_gut], n_rows[:n_gut], counts[:n_gut], tq)
    want_one = taxonomy.format_taxa_tsv(gut_cells.direct[0], gut_cells.assigned[0], gut_cells.totals[0], taxa, tq).encode()
    want_gut_reads = taxonomy.format_taxa_reads_tsv([n for n, _ in samples["gut"]], want_records[:n_gut], taxa, tq).encode()
    runs = {"plain": [], "taxa": flags[:2], "taxa_reads": flags + ["--devices", "0,0", "-j", "4"], "profile": ["--profile"],
            "profile_taxa": ["--profile"] + flags, "only": ["--profile-only"], "only_taxa": ["--profile-only"] + flags,
            "both": ["--strand", "both"], "both_taxa": ["--strand", "both"] + flags[:2]}
    for name, extra in runs.items():
        outs[name] = tmp_path / name
        outs[name].mkdir()
        _drive([driver, "-d", db_path, "-q", fasta, "-o", str(outs[name]), "--batch-size", "333"] + extra)
    one, per_read, jplace, profile_tsv = "taxa_gut.fasta.tsv", "taxa_reads_gut.fasta.tsv", "placements_gut.fasta.jplace", "profile_gut.fasta.tsv"
    for name in ("taxa", "taxa_reads", "profile_taxa", "only_taxa"):
        assert (outs[name] / one).read_bytes() == want_one, name
        assert (outs[name] / per_read).exists() == (name != "taxa"), name
        if name != "taxa":
            assert (outs[name] / per_read).read_bytes() == want_gut_reads, name
        assert not list(outs[name].glob("*.part"))
    assert not (outs["plain"] / one).exists()
    assert _without_invocation(outs["taxa"] / jplace) == _without_invocation(outs["plain"] / jplace)
    assert _without_invocation(outs["taxa_reads"] / jplace) == _without_invocation(outs["plain"] / jplace)
    assert _without_invocation(outs["profile_taxa"] / jplace) == _without_invocation(outs["profile"] / jplace)
    assert _without_invocation(outs["both_taxa"] / jplace) == _without_invocation(outs["both"] / jplace)
    assert (outs["profile_taxa"] / profile_tsv).read_bytes() == (outs["profile"] / profile_tsv).read_bytes()
    assert (outs["only_taxa"] / profile_tsv).read_bytes() == (outs["only"] / profile_tsv).read_bytes() == (outs["profile"] / profile_tsv).read_bytes()
    assert sorted(p.name for p in outs["only_taxa"].iterdir()) == sorted([one, per_read, profile_tsv])
    assert (outs["both_taxa"] / "strands_gut.fasta.tsv").read_bytes() == (outs["both"] / "strands_gut.fasta.tsv").read_bytes()
    # the launcher passes the flags on
    out_l = tmp_path / "launcher"
    out_l.mkdir()
    _drive([sys.executable, os.path.join(root, "epik.py"), "place", "-i", db_path, "-o", str(out_l), "--taxonomy",
            str(tmp_path / "taxonomy.tsv"), "--taxonomy-per-read", fasta])
    assert (out_l / one).read_bytes() == want_one and (out_l / per_read).read_bytes() == want_gut_reads


def test_drivers_taxonomy_with_mates_and_frames(placer_cls, tmp_path):
    import os
    import subprocess
    from epik_amd import dbfile, mates
    from test_profile_gpu import _write_fasta
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-C", os.path.join(root, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tq = taxonomy.mass_tau_q(0.95)
    # pairs on a nucleotide database
    tree = synth.make_tree(100, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=40, ref_length=700, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    text = synth.synth_taxonomy(tree, 4, seed=14)
    (tmp_path / "taxonomy.tsv").write_text(text)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    data, offs = synth.make_clade_reads(refs, 800, 120, seed=15)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(800)]
    first = [(f"frag_{i}/1", reads[2 * i]) for i in range(400)]
    second = [(f"frag_{i}/2", mates.reverse_complement(reads[2 * i + 1])) for i in range(400)]
    _write_fasta(str(tmp_path / "m1.fasta"), first)
    _write_fasta(str(tmp_path / "m2.fasta"), second)
    interleaved = [s for pair in zip(first, second) for _, s in pair]
    with placer_cls.from_synth(db, tree) as pl:
        rows, n_rows, counts = pl.place_mates(*synth.pack_reads(interleaved), "forward", "fr")[:3]
    records, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq)
    assert (records["taxon"] < taxa.num_taxa).sum() > 350
    want_one = taxonomy.format_taxa_tsv(cells.direct[0], cells.assigned[0], cells.totals[0], taxa, tq).encode()
    want_reads = taxonomy.format_taxa_reads_tsv([h for h, _ in first], records, taxa, tq).encode()
    flags = ["--taxonomy", str(tmp_path / "taxonomy.tsv"), "--taxonomy-per-read"]
    outs = {}
    for name, extra in (("mates", []), ("mates_taxa", flags), ("mates_only_taxa", flags + ["--profile-only", "--devices", "0,0"])):
        outs[name] = tmp_path / name
        outs[name].mkdir()
        _drive([os.path.join(root, "epik_amd", "bin", "epik-dna"), "-d", db_path, "-q", str(tmp_path / "m1.fasta"), "--mates",
                str(tmp_path / "m2.fasta"), "-o", str(outs[name]), "--batch-size", "150"] + extra)
    for name in ("mates_taxa", "mates_only_taxa"):
        assert (outs[name] / "taxa_m1.fasta.tsv").read_bytes() == want_one, name
        assert (outs[name] / "taxa_reads_m1.fasta.tsv").read_bytes() == want_reads, name
    assert _without_invocation(outs["mates_taxa"] / "placements_m1.fasta.jplace") == _without_invocation(outs["mates"] / "placements_m1.fasta.jplace")
    # translated reads on an amino-acid database
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    db_path = str(tmp_path / "aa.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    text = synth.synth_taxonomy(tree, 3, seed=9)
    (tmp_path / "aa_taxonomy.tsv").write_text(text)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(20, 200)))) for _ in range(500)] + ["AC", "NNNNNNNNNNNN"]
    named = [(f"nt_{i}", s) for i, s in enumerate(reads)]
    _write_fasta(str(tmp_path / "nt.fasta"), named)
    with placer_cls.from_synth(db, tree) as pl:
        rows, n_rows, counts = pl.place_frames(*synth.pack_reads(reads), "both")[:3]
    records, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq)
    flags = ["--taxonomy", str(tmp_path / "aa_taxonomy.tsv"), "--taxonomy-per-read"]
    for name, extra in (("frames", []), ("frames_taxa", flags)):
        outs[name] = tmp_path / name
        outs[name].mkdir()
        _drive([os.path.join(root, "epik_amd", "bin", "epik-aa"), "-d", db_path, "-q", str(tmp_path / "nt.fasta"), "--translate", "both",
                "-o", str(outs[name])] + extra)
    assert (outs["frames_taxa"] / "taxa_nt.fasta.tsv").read_bytes() == taxonomy.format_taxa_tsv(
        cells.direct[0], cells.assigned[0], cells.totals[0], taxa, tq).encode()
    assert (outs["frames_taxa"] / "taxa_reads_nt.fasta.tsv").read_bytes() == taxonomy.format_taxa_reads_tsv(
        [h for h, _ in named], records, taxa, tq).encode()
    assert (outs["frames_taxa"] / "frames_nt.fasta.tsv").read_bytes() == (outs["frames"] / "frames_nt.fasta.tsv").read_bytes()
    assert _without_invocation(outs["frames_taxa"] / "placements_nt.fasta.jplace") == _without_invocation(outs["frames"] / "placements_nt.fasta.jplace")
