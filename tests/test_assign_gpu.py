"""Placement confidence on the GPU (epik_amd_tree_*, epik_amd_confidence_device, epik_amd_placer_confidence_*,
Placer.tree / confidence_device / confidence_packed / place(assign=), epik-dna / epik-aa --assign): the device records
against the rule of include/epik_amd.h written out in test_assign_cpu.py -- bit for bit, edpl included, on the rows the
placement has just written, at the default keep_at_most and at six others, and on forged rows (test_assign_cpu.forged_batch)
at every width of the kernel's lane groups --, the same bits whatever the pieces, the stream, the grid or the chunks,
through every host entry, and the drivers' files."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import select_kernel
from epik_amd import capi, confidence, dbfile, mates, synth
from test_assign_cpu import (CLADE_BAD_ROW, CLADE_NO_HIT, CLADE_TOO_NARROW, CLADE_TOO_SHORT, FORGED_TAUS, HAND_LENGTH, HAND_PARENT,
                             RuleTree, assert_every_case_occurs, caterpillar, forged_batch, forged_tree, hand_read, numpy_rule, poison, same_bits)
from test_profile_gpu import LARGE, OTHER_KEEPS, DeviceBatch, _four_class_batch, _reads, _write_fasta, assert_profile, keep_case
from test_profile_gpu import numpy_rule as profile_rule
from test_strand_gpu import KERNELS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU_Q = confidence.tau_q(0.95)
ENV = ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_MAX_BLOCKS", "EPIK_AMD_TEAM_FRONT")


class Ladder:
    """A caterpillar tree in the shape of synth.SynthTree, as far as these tests look at one."""

    def __init__(self, n_nodes):
        self.parent, self.branch_length = caterpillar(n_nodes)
        self.num_nodes = n_nodes


@pytest.fixture(params=KERNELS + sorted(LARGE) + ["caterpillar"])
def case(request, monkeypatch, small_case):
    """(name, tree, db, reads or None): a kernel of the strand tests on the small tree, a large tree with the kernels
    create() picks, or a ladder of 9 999 branches with a clade database on it and reads of its references."""
    if request.param in LARGE or request.param == "caterpillar":
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
    if request.param in LARGE:
        tree = synth.make_tree(LARGE[request.param], seed=30)
        return request.param, tree, synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7), None
    if request.param == "caterpillar":
        tree = Ladder(9999)
        db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=60, ref_length=600, seed=14)
        data, offs = synth.make_clade_reads(refs, 500, 150, seed=15)
        reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(500)]
        return request.param, tree, db, reads + ["ACG", "", "N" * 30, "ACGTTGCATGCATGACGT"]
    select_kernel(monkeypatch, request.param)
    return (request.param,) + tuple(small_case) + (None,)


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def device_records(pl, tree, batch, tau_q, first=0, count=None, stream=None, out=None):
    """confidence_device on (a piece of) the rows a DeviceBatch holds; the records as a numpy array."""
    torch = batch.torch
    keep = pl.keep_at_most
    count = batch.n - first if count is None else count
    stream = batch.stream if stream is None else stream
    if out is None:
        out = torch.full((batch.n * 2,), float("nan"), dtype=torch.float64, device=batch.d_rows.device)
        torch.cuda.synchronize()
    pl.confidence_device(tree, batch.d_rows.data_ptr() + first * keep * 16, batch.d_n.data_ptr() + first * 4,
                         batch.d_counts.data_ptr() + first * keep * 4, count, tau_q, out.data_ptr() + first * 16, stream.cuda_stream)
    return out


def records_of(out):
    import torch
    torch.cuda.synchronize()
    return out.cpu().numpy().view(capi.CONFIDENCE)


def test_confidence_device_equals_the_rule_on_the_rows_just_written(placer_cls, case):
    name, tree, db, reads = case
    rng = np.random.default_rng(11)
    with placer_cls.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        if reads is None:
            reads, _ = _four_class_batch(pl, db.kmer_size, rng)
        else:
            pl.choose_counts(200)
        assert len(reads) % 64 != 0
        info = tr.info()
        assert info["num_branches"] == db.num_branches and info["levels"] == max(1, int(np.ceil(np.log2(db.num_branches))))
        assert info["table_bytes"] == 32 + db.num_branches * (16 + 8 * info["levels"]) + (4 * db.num_branches + 7) // 8 * 8
        batch = DeviceBatch(pl, reads)                    # (the slots past n_rows are poisoned: NaN rows, counts of 3)
        rows, n_rows, counts = batch.host()
        rule = RuleTree(tree.parent, tree.branch_length)
        for tau in (0.95, 0, 0.5, 1):
            got = records_of(device_records(pl, tr, batch, confidence.tau_q(tau)))
            want = numpy_rule(rule, rows, n_rows, counts, confidence.tau_q(tau))
            assert same_bits(got, want), (name, tau, np.nonzero(got != want)[0][:10])
        ok = want["clade"] < db.num_branches
        classes = {c: int((want["clade"] == c).sum()) for c in (CLADE_TOO_NARROW, CLADE_TOO_SHORT, CLADE_NO_HIT, CLADE_BAD_ROW)}
        print(name, "placed", int(ok.sum()), "classes", classes, "max edpl", float(want["edpl"].max()))
        assert ok.sum() > 100 and classes[CLADE_TOO_SHORT] > 0 and classes[CLADE_BAD_ROW] == 0
        if name != "caterpillar":
            assert classes[CLADE_NO_HIT] > 0 and classes[CLADE_TOO_NARROW] > 0
        several = int((n_rows[ok] >= 2).sum())
        assert (several > 0 if name == "caterpillar" else several * 2 >= ok.sum()) and want["edpl"].max() > 0


@pytest.mark.parametrize("tree_name", ["small", "tree3999"])
def test_same_bits_whatever_the_pieces_the_stream_the_grid_and_the_chunks(placer_cls, small_case, monkeypatch, tree_name):
    import torch
    if tree_name == "small":
        select_kernel(monkeypatch, "paired")
        tree, db = small_case
    else:
        for var in ENV:
            monkeypatch.delenv(var, raising=False)
        tree = synth.make_tree(LARGE[tree_name], seed=30)
        db = synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)
    reads = _reads(db.kmer_size, np.random.default_rng(21), 3000)
    data, offs = synth.pack_reads(reads)
    results = {}
    for name, env in (("one call", {}), ("uneven pieces", {}), ("two streams", {}), ("two workgroups", {"EPIK_AMD_MAX_BLOCKS": "2"}),
                      ("host entry", {}), ("host entry, chunks of five", {"EPIK_AMD_CONFIDENCE_CHUNK_READS": "5"})):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        with placer_cls.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
            if name.startswith("host entry"):
                part = slice(0, 333) if "chunks" in name else slice(None)
                rows, n_rows, counts, label, conf = pl.confidence_packed(tr, *synth.pack_reads(reads[part]), TAU_Q)
                plain = pl.place_packed(*synth.pack_reads(reads[part]))
                assert label is None and all(a.tobytes() == b.tobytes() for a, b in zip((rows, n_rows, counts), plain))
                results[name] = (conf, part)
                # ... and with the rows left on the device
                none = pl.confidence_packed(tr, *synth.pack_reads(reads[part]), TAU_Q, rows_out=False)
                assert none[:4] == (None, None, None, None) and same_bits(none[4], conf)
            else:
                pl.choose_counts(200)
                batch = DeviceBatch(pl, reads)
                if name == "uneven pieces":
                    out = None
                    cuts = [0, 1, 64, 65, 700, 701, 2999, len(reads)]
                    for a, b in zip(cuts, cuts[1:]):
                        out = device_records(pl, tr, batch, TAU_Q, a, b - a, out=out)
                    device_records(pl, tr, batch, TAU_Q, 5, 0, out=out)          # n == 0: nothing
                elif name == "two streams":
                    out = device_records(pl, tr, batch, TAU_Q, 0, 1500)
                    device_records(pl, tr, batch, TAU_Q, 1500, None, torch.cuda.Stream(), out=out)
                else:
                    out = device_records(pl, tr, batch, TAU_Q)
                results[name] = (records_of(out), slice(None))
                if name == "one call":
                    want = numpy_rule(RuleTree(tree.parent, tree.branch_length), *batch.host(), TAU_Q)
        for key in env:
            monkeypatch.delenv(key)
    for name, (got, part) in results.items():
        assert same_bits(got, want[part]), (name, np.nonzero(got != want[part])[0][:10])
    del data, offs


def test_strands_and_mates_entries_equal_the_rule_on_the_placed_rows(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    tree, db = small_case
    rng = np.random.default_rng(31)
    reads = _reads(db.kmer_size, rng, 1200)
    reads += reads[:len(reads) % 2]
    weights = rng.integers(0, 9, size=len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    rule = RuleTree(tree.parent, tree.branch_length)
    with placer_cls.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as tr, pl.profile() as profile, pl.profile() as ref:
        for kind, mode, env in (("strand", "both", "EPIK_AMD_STRAND_CHUNK_READS"), ("strand", "reverse", None),
                                ("mates", "fr", "EPIK_AMD_MATES_CHUNK_READS"), ("mates", "ff", None)):
            if kind == "strand":
                placed = pl.place_strands(data, offs, mode)
                kw, w = dict(strand=mode), weights
            else:
                placed = pl.place_mates(data, offs, "both", mode)
                kw, w = dict(strand="both", mates=mode), weights[:len(reads) // 2]
            want = numpy_rule(rule, placed[0], placed[1], placed[2], TAU_Q)
            assert (want["clade"] < db.num_branches).sum() > 100
            for chunk in (None, "5") if env else (None,):
                if chunk:
                    monkeypatch.setenv(env, chunk)
                profile.reset()
                got = pl.confidence_packed(tr, data, offs, TAU_Q, profile=profile, weights=w, **kw)
                if chunk:
                    monkeypatch.delenv(env)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], placed)), (kind, mode, chunk)
                assert same_bits(got[4], want), (kind, mode, chunk, np.nonzero(got[4] != want)[0][:10])
                # the profile chained to the same rows holds the bits of profile_packed
                ref.reset()
                labels = pl.profile_packed(ref, data, offs, w, **kw)
                assert np.array_equal(labels, placed[3])
                assert_profile(profile.read(), profile_rule(placed[0], placed[1], placed[2], w, db.num_branches), f"{kind} {mode} {chunk}")
                got_ref = ref.read()
                assert np.array_equal(profile.read().mass, got_ref.mass) and profile.read().totals == got_ref.totals
        # a tree of another shape, a tau_q beyond 2^30 and a profile of another shape are refused
        with pl.tree(*caterpillar(db.num_branches)) as other:
            pl.confidence_packed(other, data, offs, TAU_Q)          # (same size: accepted; the tree is the caller's)
        with placer_cls.from_synth(db, keep_at_most=3) as small, pytest.raises(capi.EpikAmdError) as e:
            small.confidence_packed(tr, data, offs, TAU_Q, profile=profile)
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(capi.EpikAmdError) as e:
            pl.confidence_packed(tr, data, offs, (1 << 30) + 1)
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(ValueError):
            pl.tree(tree.parent[:-2], tree.branch_length[:-2])


def test_frames_entry_equals_the_rule_on_the_placed_rows(placer_cls, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT" if i % 3 else "ACGTUNRYKMSWBDHV-."), size=int(rng.integers(0, 200)))) for i in range(700)]
    reads += ["", "AC", "TAATAGTGATAATAGTGA", "NNNNNNNNNNNN"]
    weights = rng.integers(0, 9, size=len(reads)).astype(np.uint32)
    data, offs = synth.pack_reads(reads)
    with placer_cls.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as tr, pl.profile() as profile:
        placed = pl.place_frames(data, offs, "both")
        want = numpy_rule(RuleTree(tree.parent, tree.branch_length), placed[0], placed[1], placed[2], TAU_Q)
        assert (want["clade"] < db.num_branches).sum() > 100 and (want["clade"] == CLADE_TOO_SHORT).sum() > 0
        for chunk in (None, "5"):
            if chunk:
                monkeypatch.setenv("EPIK_AMD_FRAME_CHUNK_READS", chunk)
            profile.reset()
            got = pl.confidence_packed(tr, data, offs, TAU_Q, profile=profile, weights=weights, translate="both")
            monkeypatch.delenv("EPIK_AMD_FRAME_CHUNK_READS", raising=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:4], placed)), chunk
            assert same_bits(got[4], want), chunk
            assert_profile(profile.read(), profile_rule(placed[0], placed[1], placed[2], weights, db.num_branches), f"frames {chunk}")
        with pytest.raises(capi.EpikAmdError) as e:          # strands need a nucleotide handle
            pl.confidence_packed(tr, data, offs, TAU_Q, strand="both")
        assert e.value.code == capi.ERR_UNSUPPORTED


def test_place_returns_the_records_beside_the_rows(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree, db = small_case
    reads = _reads(db.kmer_size, np.random.default_rng(5), 100)
    records = [(f"r{i}", s) for i, s in enumerate(reads)] + [(f"d{i}", reads[i % 7]) for i in range(40)]
    with placer_cls.from_synth(db, tree) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        plain = pl.place(records)
        placed = pl.place(records, assign=0.95, tree=tr)
        assert placed == plain and plain.confidence is None and len(placed.confidence) == len(placed.placed_seqs)
        rows, n_rows, counts = pl.place_packed(*synth.pack_reads([s.sequence for s in placed.placed_seqs]))
        assert same_bits(placed.confidence, numpy_rule(RuleTree(tree.parent, tree.branch_length), rows, n_rows, counts, TAU_Q))
        both = pl.place(records, strand="both", assign=0.5, tree=tr)
        assert both == pl.place(records, strand="both") and len(both.confidence) == len(both.placed_seqs)
        with pytest.raises(ValueError):
            pl.place(records, assign=0.95)


def _expected_files(pl, tr, tree, records, batch, tau, **place_kw):
    """Both files as the drivers write them, from Placer.place over the driver's batches (dedup per batch, place.cpp:207)."""
    names, conf = [], []
    for first in range(0, len(records), batch):
        part = records[first:first + batch]
        placed = pl.place(part, assign=tau, tree=tr, **place_kw)
        index = {s.sequence: i for i, s in enumerate(placed.placed_seqs)}
        for header, sequence in part:
            names.append(header)
            conf.append(placed.confidence[index[sequence]])
    conf = np.array(conf, dtype=capi.CONFIDENCE)
    sizes = confidence.subtree_sizes(tree.parent)
    tq = confidence.tau_q(tau)
    assigned, classes = confidence.clade_counts(conf, None, len(sizes))
    return (confidence.format_assign_tsv(names, conf, sizes, tq).encode(), confidence.format_clades_tsv(assigned, classes, sizes, tq).encode(), conf)


def _without_invocation(path):
    lines = path.read_bytes().split(b"\n")
    quoted = [i for i, line in enumerate(lines) if b'"invocation"' in line]
    assert len(quoted) == 1
    del lines[quoted[0]]
    return lines


def test_drivers_write_the_assign_files(placer_cls, tmp_path):
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
    records = [(f"read_{i} sample", s) for i, s in enumerate(reads)]
    fasta = str(tmp_path / "sample.fasta")
    _write_fasta(fasta, records)
    batch = 777
    with placer_cls.from_synth(db, tree) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        want_assign, want_clades, conf = _expected_files(pl, tr, tree, records, batch, 0.95)
        want_half = _expected_files(pl, tr, tree, records, batch, 0.5)
        want_both = _expected_files(pl, tr, tree, records, batch, 0.95, strand="both")
    ok = conf["clade"] < db.num_branches
    assert ok.sum() > 3000 and (conf["clade"] == CLADE_NO_HIT).sum() > 0 and (conf["clade"] == CLADE_TOO_SHORT).sum() == 3
    assert (conf["edpl"][ok] > 0).sum() > 100
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    runs = {"plain": [], "assign_j1": ["--assign", "-j", "1"], "assign_j16": ["--assign", "-j", "16"],
            "assign_two_handles": ["--assign", "--devices", "0,0", "-j", "4"], "assign_half": ["--assign", "--assign-mass", "0.5"],
            "only": ["--profile-only", "--assign"], "only_two_handles": ["--profile-only", "--assign", "--devices", "0,0", "-j", "4"],
            "profile": ["--profile"], "profile_assign": ["--profile", "--assign"], "profile_only": ["--profile-only"],
            "both": ["--strand", "both", "--profile"], "both_assign": ["--strand", "both", "--profile", "--assign"],
            "both_only_assign": ["--strand=both", "--profile-only", "--assign"]}
    outs = {}
    for name, extra in runs.items():
        outs[name] = tmp_path / name
        outs[name].mkdir()
        run = subprocess.run([driver, "-d", db_path, "-q", fasta, "-o", str(outs[name]), "--batch-size", str(batch)] + extra,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, name + run.stdout[-2000:] + run.stderr[-2000:]
    assign, clades, jplace = "assign_sample.fasta.tsv", "assign_clades_sample.fasta.tsv", "placements_sample.fasta.jplace"
    profile_tsv, strands = "profile_sample.fasta.tsv", "strands_sample.fasta.tsv"
    assert not (outs["plain"] / assign).exists() and not (outs["plain"] / clades).exists()
    for name in ("assign_j1", "assign_j16", "assign_two_handles", "only", "only_two_handles", "profile_assign"):
        assert (outs[name] / assign).read_bytes() == want_assign, name
        assert (outs[name] / clades).read_bytes() == want_clades, name
        assert not (outs[name] / (assign + ".part")).exists()
        assert (outs[name] / jplace).exists() == (not name.startswith("only")), name
    assert (outs["assign_half"] / assign).read_bytes() == want_half[0] != want_assign
    assert (outs["assign_half"] / clades).read_bytes() == want_half[1]
    for name in ("both_assign", "both_only_assign"):
        assert (outs[name] / assign).read_bytes() == want_both[0], name
        assert (outs[name] / clades).read_bytes() == want_both[1], name
    # everything else a run writes is what it is without --assign
    assert _without_invocation(outs["assign_j1"] / jplace) == _without_invocation(outs["plain"] / jplace)
    assert _without_invocation(outs["profile_assign"] / jplace) == _without_invocation(outs["profile"] / jplace)
    assert _without_invocation(outs["both_assign"] / jplace) == _without_invocation(outs["both"] / jplace)
    assert (outs["profile_assign"] / profile_tsv).read_bytes() == (outs["profile"] / profile_tsv).read_bytes()
    assert (outs["only"] / profile_tsv).read_bytes() == (outs["profile_only"] / profile_tsv).read_bytes() == (outs["profile"] / profile_tsv).read_bytes()
    assert (outs["both_assign"] / profile_tsv).read_bytes() == (outs["both"] / profile_tsv).read_bytes() == (outs["both_only_assign"] / profile_tsv).read_bytes()
    assert (outs["both_assign"] / strands).read_bytes() == (outs["both"] / strands).read_bytes() == (outs["both_only_assign"] / strands).read_bytes()
    assert sorted(p.name for p in outs["only"].iterdir()) == sorted([assign, clades, profile_tsv])
    # the launcher passes the flags on
    out_l = tmp_path / "launcher"
    out_l.mkdir()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(out_l), "--profile-only",
                          "--assign", "--assign-mass", "0.5", fasta], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    back = confidence.read_assign_tsv(str(out_l / assign))
    assert back["tau_q"] == 1 << 29 and back["records"] == len(records) and back["names"] == [h for h, _ in records]
    sums = confidence.read_clades_tsv(str(out_l / clades))
    assert sums["records"] == len(records) and int(sums["clade_assigned"][-1]) == sums["assigned_records"]


def test_drivers_assign_with_mates_and_frames(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    # pairs on a nucleotide database
    tree = synth.make_tree(200, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=40, ref_length=700, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    data, offs = synth.make_clade_reads(refs, 1200, 120, seed=15)
    reads = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(1200)]
    first = [(f"frag_{i}/1", reads[2 * i]) for i in range(600)]
    second = [(f"frag_{i}/2", mates.reverse_complement(reads[2 * i + 1])) for i in range(600)]
    _write_fasta(str(tmp_path / "m1.fasta"), first)
    _write_fasta(str(tmp_path / "m2.fasta"), second)
    with placer_cls.from_synth(db, tree) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        names, conf = [], []
        for at in range(0, 600, 250):
            placed = pl.place(first[at:at + 250], mates=second[at:at + 250], assign=0.95, tree=tr)
            index = {(s.sequence, s.mate): i for i, s in enumerate(placed.placed_seqs)}
            for (header, a), (_, b) in zip(first[at:at + 250], second[at:at + 250]):
                names.append(header)
                conf.append(placed.confidence[index[(a, b)]])
    conf = np.array(conf, dtype=capi.CONFIDENCE)
    sizes = confidence.subtree_sizes(tree.parent)
    assert (conf["clade"] < db.num_branches).sum() > 500
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    outs = {}
    for name, extra in (("mates", []), ("mates_assign", ["--assign"]), ("mates_only_assign", ["--assign", "--profile-only"])):
        outs[name] = tmp_path / name
        outs[name].mkdir()
        run = subprocess.run([driver, "-d", db_path, "-q", str(tmp_path / "m1.fasta"), "--mates", str(tmp_path / "m2.fasta"), "-o",
                              str(outs[name]), "--batch-size", "250"] + extra, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, name + run.stdout[-2000:] + run.stderr[-2000:]
    for name in ("mates_assign", "mates_only_assign"):
        assert (outs[name] / "assign_m1.fasta.tsv").read_bytes() == confidence.format_assign_tsv(names, conf, sizes, TAU_Q).encode(), name
    assert _without_invocation(outs["mates_assign"] / "placements_m1.fasta.jplace") == _without_invocation(outs["mates"] / "placements_m1.fasta.jplace")
    # translated reads on an amino-acid database
    tree = synth.make_tree(30, seed=8)
    db = synth.make_db(tree.num_nodes, states="amino", kmer_size=4, seed=12, p_present=0.4, lognormal=(1.5, 1.0))
    db_path = str(tmp_path / "aa.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    rng = np.random.default_rng(41)
    reads = ["".join(rng.choice(list("ACGT"), size=int(rng.integers(20, 200)))) for _ in range(500)] + ["AC", "NNNNNNNNNNNN"]
    records = [(f"nt_{i}", s) for i, s in enumerate(reads)]
    _write_fasta(str(tmp_path / "nt.fasta"), records)
    with placer_cls.from_synth(db, tree) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        placed = pl.place(records, translate="both", assign=0.95, tree=tr)
        index = {s.sequence: i for i, s in enumerate(placed.placed_seqs)}
        conf = np.array([placed.confidence[index[s]] for _, s in records], dtype=capi.CONFIDENCE)
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-aa")
    for name, extra in (("frames", []), ("frames_assign", ["--assign"])):
        outs[name] = tmp_path / name
        outs[name].mkdir()
        run = subprocess.run([driver, "-d", db_path, "-q", str(tmp_path / "nt.fasta"), "--translate", "both", "-o", str(outs[name])] + extra,
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, name + run.stdout[-2000:] + run.stderr[-2000:]
    want = confidence.format_assign_tsv([h for h, _ in records], conf, confidence.subtree_sizes(tree.parent), TAU_Q).encode()
    assert (outs["frames_assign"] / "assign_nt.fasta.tsv").read_bytes() == want
    assert (outs["frames_assign"] / "frames_nt.fasta.tsv").read_bytes() == (outs["frames"] / "frames_nt.fasta.tsv").read_bytes()
    assert _without_invocation(outs["frames_assign"] / "placements_nt.fasta.jplace") == _without_invocation(outs["frames"] / "placements_nt.fasta.jplace")


# ---- forged rows: confidence_kernel at every group width, on every class and edge of the rule -------------------------
#: every group width P of the kernel once exactly filled and once with idle lanes, on a binary and a multifurcating tree
WIDTH_KEEPS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 32, 33, 63, 64)
#: ... and every tree at three widths; the ladder has 14 lift levels, and pairs that lie far apart
FORGED_TREE_NAMES = ("one_branch", "hand", "multifurcating", "star300", "synth500", "ladder9999")
FORGED_CASES = sorted({(t, k) for t in ("synth500", "multifurcating") for k in WIDTH_KEEPS} | {(t, k) for t in FORGED_TREE_NAMES for k in (7, 13, 64)})
FORGED = {}


def per_block(keep):
    """The reads of a tile of confidence_kernel: 256 lanes in groups of P, the power of two >= keep."""
    group = 1
    while group < keep:
        group *= 2
    return 256 // group


class ForgedCase:
    """A forged batch on one tree at one keep, made once; the restatement's records per tau_q, computed once each and
    left as they are.  n is no multiple of the tile: the last tile of a launch is partial."""

    def __init__(self, tree_name, keep, n=None):
        self.keep, self.n = keep, n or (1000 if keep <= 16 else 301)
        assert self.n % per_block(keep) != 0
        self.parent, self.lengths, self.rule = forged_tree(tree_name)
        self.rows, self.n_rows, self.counts = forged_batch(np.random.default_rng([keep, len(self.parent)]), self.n, keep, len(self.parent))
        self.wants = {}

    def want(self, tq):
        if tq not in self.wants:
            self.wants[tq] = numpy_rule(self.rule, self.rows, self.n_rows, self.counts, tq)
            assert_every_case_occurs(self.rule, self.rows, self.n_rows, self.counts, tq, self.wants[tq])
        return self.wants[tq]


def forged_case(tree_name, keep, n=None):
    if (tree_name, keep, n) not in FORGED:
        FORGED[tree_name, keep, n] = ForgedCase(tree_name, keep, n)
    return FORGED[tree_name, keep, n]


class ForgedDevice:
    """Host rows in torch buffers on the device, and an output of n + 8 records filled with NaN."""

    def __init__(self, rows, n_rows, counts):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n, self.keep = rows.shape
        self.d_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.float64).reshape(-1)).to(dev)
        self.d_n = torch.from_numpy(np.ascontiguousarray(n_rows, dtype=np.uint32).view(np.int32)).to(dev)
        self.d_counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
        self.stream = torch.cuda.Stream()
        self.fresh()

    def fresh(self):
        self.out = self.torch.full((2 * (self.n + 8),), float("nan"), dtype=self.torch.float64, device=self.d_rows.device)
        self.before = self.out.cpu().numpy().copy()
        self.torch.cuda.synchronize()

    def run(self, tree, tq, first=0, count=None):
        count = self.n - first if count is None else count
        tree.confidence_device(self.d_rows.data_ptr() + first * self.keep * 16, self.d_n.data_ptr() + first * 4,
                               self.d_counts.data_ptr() + first * self.keep * 4, count, self.keep, tq,
                               self.out.data_ptr() + first * 16, self.stream.cuda_stream)

    def records(self, written):
        """The first `written` records; every record past them must be as it was."""
        self.stream.synchronize()
        got = self.out.cpu().numpy()
        assert np.array_equal(got[2 * written:].view(np.uint64), self.before[2 * written:].view(np.uint64)), "a record past n was written"
        return got[:2 * written].view(capi.CONFIDENCE)


def poisoned(rows, n_rows, counts):
    rows, counts = poison(rows, n_rows, counts)
    return rows, n_rows, counts


@pytest.fixture
def forged_env(gpu_available, monkeypatch):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    return monkeypatch


def differing(got, want):
    return np.nonzero(got.view(np.uint64).reshape(-1, 2) != want.view(np.uint64).reshape(-1, 2))[0][:10]


@pytest.mark.parametrize("tq", FORGED_TAUS)
@pytest.mark.parametrize("tree_name,keep", FORGED_CASES)
def test_confidence_kernel_equals_the_rule_on_forged_rows(forged_env, tree_name, keep, tq):
    case = forged_case(tree_name, keep)
    want = case.want(tq)
    batch = ForgedDevice(case.rows, case.n_rows, case.counts)
    with confidence.Tree(0, case.parent, case.lengths) as tr:
        batch.run(tr, tq)
        got = batch.records(case.n)
        assert same_bits(got, want), (tree_name, keep, tq, differing(got, want))
        # one read; one read more than a tile
        for n in (1, per_block(keep) + 1):
            batch.fresh()
            batch.run(tr, tq, 0, n)
            got = batch.records(n)
            assert same_bits(got, want[:n]), (tree_name, keep, tq, n, differing(got, want[:n]))


@pytest.mark.parametrize("keep,n", [(1, 5001), (64, None)])
def test_forged_rows_under_two_workgroups(forged_env, keep, n):
    """EPIK_AMD_MAX_BLOCKS is read when the tree is created: a workgroup then walks many tiles of the grid stride (ten
    of 256 reads at keep 1, thirty-eight of 4 at keep 64; the last one partial)."""
    case = forged_case("synth500", keep, n)
    assert (case.n + per_block(keep) - 1) // per_block(keep) >= 20
    batch = ForgedDevice(case.rows, case.n_rows, case.counts)
    forged_env.setenv("EPIK_AMD_MAX_BLOCKS", "2")
    with confidence.Tree(0, case.parent, case.lengths) as tr:
        for tq in (FORGED_TAUS[1], FORGED_TAUS[2]):
            batch.fresh()
            batch.run(tr, tq)
            got = batch.records(case.n)
            assert same_bits(got, case.want(tq)), (keep, tq, differing(got, case.want(tq)))


@pytest.mark.parametrize("keep", [3, 7, 64])
def test_forged_rows_in_uneven_pieces(forged_env, keep):
    case = forged_case("multifurcating", keep)
    cuts = [0, 1, 6, 7, 101, 102, 299, case.n]
    assert all(c % per_block(keep) for c in cuts[1:]) and any((b - a) > per_block(keep) for a, b in zip(cuts, cuts[1:]))
    batch = ForgedDevice(case.rows, case.n_rows, case.counts)
    with confidence.Tree(0, case.parent, case.lengths) as tr:
        for a, b in zip(cuts, cuts[1:]):
            batch.run(tr, TAU_Q, a, b - a)
        batch.run(tr, TAU_Q, 5, 0)                           # n == 0: nothing
        got = batch.records(case.n)
    assert same_bits(got, case.want(TAU_Q)), (keep, differing(got, case.want(TAU_Q)))


@pytest.mark.parametrize("keep", [3, 7, 64])
def test_hand_values_on_the_device(forged_env, keep):
    rows, n_rows, counts = hand_read(keep)
    with confidence.Tree(0, HAND_PARENT, HAND_LENGTH) as tr:
        batch = ForgedDevice(*poisoned(rows, n_rows, counts))
        for tau, clade, mass in ((0.5, 0, 1 << 29), (0.75, 2, 3 << 28), (0.95, 6, 1 << 30)):
            batch.fresh()
            batch.run(tr, confidence.tau_q(tau))
            got = batch.records(1)[0]
            assert (int(got["clade"]), int(got["clade_mass_q"]), float(got["edpl"])) == (clade, mass, 4.75), tau
        # one row: +0.0, the clade is the branch whatever tau
        rows["branch"][0, 0], n_rows[0] = 4, 1
        batch = ForgedDevice(*poisoned(rows, n_rows, counts))
        batch.run(tr, 1 << 30)
        got = batch.records(1)
        assert int(got["clade"][0]) == 4 and got["edpl"].view(np.uint64)[0] == 0 and int(got["clade_mass_q"][0]) == 1 << 29


@pytest.mark.parametrize("keep", [0, 65])
def test_a_keep_outside_1_to_64_is_refused(forged_env, keep):
    rows, n_rows, counts = hand_read(7)
    batch = ForgedDevice(rows, n_rows, counts)
    with confidence.Tree(0, HAND_PARENT, HAND_LENGTH) as tr:
        with pytest.raises(capi.EpikAmdError) as e:
            tr.confidence_device(batch.d_rows.data_ptr(), batch.d_n.data_ptr(), batch.d_counts.data_ptr(), 1, keep, TAU_Q,
                                 batch.out.data_ptr(), batch.stream.cuda_stream)
        assert e.value.code == capi.ERR_INVALID and "keep" in str(e.value)
    assert len(batch.records(0)) == 0                       # nothing was written


# ---- other keep_at_most: the rows a placement wrote at that keep ------------------------------------------------------
@pytest.mark.parametrize("tq", [1 << 29, TAU_Q])
@pytest.mark.parametrize("keep", OTHER_KEEPS)
def test_confidence_device_at_other_keep_at_most(placer_cls, monkeypatch, keep, tq):
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    tree, db = keep_case()
    reads = _reads(db.kmer_size, np.random.default_rng(keep), 600)
    with placer_cls.from_synth(db, keep_at_most=keep) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        assert pl.keep_at_most == keep
        pl.choose_counts(200)
        batch = DeviceBatch(pl, reads)
        rows, n_rows, counts = batch.host()
        assert rows.shape == (len(reads), keep)
        got = records_of(device_records(pl, tr, batch, tq))[:len(reads)]
    want = numpy_rule(RuleTree(tree.parent, tree.branch_length), rows, n_rows, counts, tq)
    assert same_bits(got, want), (keep, tq, differing(got, want))
    ok = want["clade"] < db.num_branches
    print(f"keep {keep}: {int(ok.sum())} placed reads, at most {int(n_rows[ok].max())} rows, {int((n_rows[ok] == keep).sum())} reads of keep rows")
    assert ok.sum() > 100 and (want["clade"] == CLADE_BAD_ROW).sum() == 0 and (want["clade"] == CLADE_TOO_SHORT).sum() > 0
    assert (n_rows[ok] == keep).sum() > 0                   # (the CPU oracle fills all 64 rows for a third of these reads)
