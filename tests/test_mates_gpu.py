"""Paired-end placement on the GPU (epik_amd_placer_place_mates[_device], epik_amd_placer_profile_mates,
Placer.place_mates, epik-dna --mates): the placement of a pair is the CPU oracle's placement of the joined sequence
J = m1 . sep . rc(m2) built on the host, bit for bit; the strand modes are the strand placement's on J; the device and
the host entry, the chunks and the profile agree; the drivers write one placement per fragment."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_rows_match, mixed_reads, select_kernel
from epik_amd import capi, dbfile, jplace, jplace_diff, mates, synth
from test_profile_gpu import assert_profile, numpy_rule
from test_strand_gpu import KERNELS, both_rule, has_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rc = mates.reverse_complement


@pytest.fixture(params=KERNELS)
def kernel(request, monkeypatch):
    select_kernel(monkeypatch, request.param)
    return request.param


@pytest.fixture(scope="module")
def placer_cls(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"
    from epik_amd.placer import Placer
    return Placer


def _pairs(k, rng, n=300):
    """(mate 1, mate 2) pairs: mixed reads, and the cases the rule has to get right at the junction."""
    reads = mixed_reads(rng, 2 * n, k, alphabet_amb="ACGTNRYKMSWBDHV-", max_len=120)
    reads = [r.lower() if i % 7 == 0 else r for i, r in enumerate(reads)]
    pairs = list(zip(reads[0::2], reads[1::2]))
    long_a, long_b = ("".join(rng.choice(list("ACGT"), size=150)) for _ in range(2))
    pairs += [("", "ACGTACGTACGGT"), ("ACGTACGTACGGT", ""), ("", ""),        # an empty mate on either side, both
              ("AC", "GT"), ("A", ""), ("ACG", "ACGTTGCATG"), ("ACGTTGCATG", "CG"),   # mates shorter than k
              ("ACGTTGCAN", "NACGTTGCA"), ("ACGTTGCAR", "YACGTTGCA"),         # ambiguous characters next to the junction
              ("ACGTTGCA-", "-ACGTTGCA"), ("ACGTTGCA*", ".ACGTTGCA"),         # invalid ones
              ("acgttgcatg", "ttgaccgtua"), ("ACGUACGUUUAC", "UUGACCA"),      # lower case, U
              (long_a, long_b), (long_b, rc(long_a)),                         # 2 x 150 bp: 16-bit counts
              ("ACGTACGT", "ACGTACGT"), ("ACGT" * 6, "ACGT" * 6)]             # palindromes
    return pairs


def _joined(pairs, orientation="fr", sep="-"):
    return [mates.join(a, b, orientation, sep) for a, b in pairs]


def _pack(pairs):
    return mates.interleave([a for a, _ in pairs], [b for _, b in pairs])


def _oracle(orc, reads):
    return orc.place(*synth.pack_reads(reads), num_threads=0)


def _same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("orientation", ["fr", "ff"])
def test_forward_equals_the_oracle_on_the_joined_sequences(placer_cls, oracle_lib, small_case, kernel, orientation):
    _, db = small_case
    pairs = _pairs(db.kmer_size, np.random.default_rng(1))
    data, offs = _pack(pairs)
    with placer_cls.from_synth(db) as pl:
        sep = chr(pl.mates_separator())
        rows, n, counts, strand = pl.place_mates(data, offs, "forward", orientation)
    assert sep == "-"
    want = _oracle(oracle_lib.Oracle.from_synth(db), _joined(pairs, orientation, sep))
    assert_rows_match(rows, n, counts, *want)
    assert not strand.any() and len(n) == len(pairs)
    # a pair whose mates are both shorter than k while J is not: a read without hits, not a read too short
    i = pairs.index(("AC", "GT"))
    assert n[i] > 0 and not counts[i].any()
    assert n[pairs.index(("A", ""))] == 0 and n[pairs.index(("", ""))] == 0


@pytest.mark.parametrize("orientation", ["fr", "ff"])
def test_reverse_and_both_equal_the_strand_rule_on_two_oracle_runs(placer_cls, oracle_lib, small_case, kernel, orientation):
    _, db = small_case
    pairs = _pairs(db.kmer_size, np.random.default_rng(2))
    pairs += [(b, a) for a, b in pairs[:40]]          # the same fragments read from the other strand
    data, offs = _pack(pairs)
    joined = _joined(pairs, orientation)
    orc = oracle_lib.Oracle.from_synth(db)
    fwd, rev = _oracle(orc, joined), _oracle(orc, [rc(j) for j in joined])
    want, want_strand = both_rule(fwd, rev)
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, strand = pl.place_mates(data, offs, "reverse", orientation)
        assert_rows_match(rows, n, counts, *rev)
        assert (strand == 1).all()
        rows, n, counts, strand = pl.place_mates(data, offs, "both", orientation)
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(strand, want_strand)
    assert 0 < int(strand.sum()) < len(pairs)


def test_swapping_the_mates_flips_the_strand_and_keeps_the_rows(placer_cls, small_case, kernel):
    _, db = small_case
    pairs = _pairs(db.kmer_size, np.random.default_rng(3))
    with placer_cls.from_synth(db) as pl:
        fwd = pl.place_mates(*_pack(pairs), "forward")
        rev = pl.place_mates(*_pack(pairs), "reverse")
        rows, n, counts, strand = pl.place_mates(*_pack(pairs), "both")
        s_rows, s_n, s_counts, s_strand = pl.place_mates(*_pack([(b, a) for a, b in pairs]), "both")
    placed = has_rows(fwd[1]) & has_rows(rev[1])
    differ = placed & (fwd[0]["score"][:, 0].view(np.uint32) != rev[0]["score"][:, 0].view(np.uint32))
    assert differ.sum() > 100
    assert np.array_equal(s_strand[differ], 1 - strand[differ])
    assert not strand[~differ].any() and not s_strand[~differ].any()      # a tie, or no rows: forward
    same = differ | ~placed
    assert rows[same].tobytes() == s_rows[same].tobytes() and n[same].tobytes() == s_n[same].tobytes()
    assert counts[same].tobytes() == s_counts[same].tobytes()


def _device_run(pl, data, offs, strand, orientation, stream, ws_bytes=None, guard=0):
    import torch
    dev = torch.device("cuda", pl.device)
    n, keep, seq_bytes = (len(offs) - 1) // 2, pl.keep_at_most, int(offs[-1])
    d_seqs = torch.from_numpy(np.ascontiguousarray(data)).to(dev) if len(data) else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_offs = torch.from_numpy(np.ascontiguousarray(offs).view(np.int64)).to(dev)
    d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
    d_n = torch.zeros(n, dtype=torch.int32, device=dev)
    d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
    d_strand = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = pl.mates_workspace_bytes(n, seq_bytes, strand, orientation) if ws_bytes is None else ws_bytes
    # (zeroed, as the host entry has it: in `both` the row slots past n_rows of a pair whose reverse strand wins are
    # those of the reverse rows, which lie in the workspace)
    d_ws = torch.zeros(ws + guard, dtype=torch.uint8, device=dev)
    d_ws[ws:] = 0xA5
    torch.cuda.synchronize()
    pl.place_mates_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, seq_bytes, strand, orientation, d_ws.data_ptr(), ws,
                          d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_strand.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    if guard:
        assert bool((d_ws[ws:] == 0xA5).all()), "the guard band behind the workspace was written"
    return (d_rows.cpu().numpy().view(capi.PLACEMENT).reshape(n, keep), d_n.cpu().numpy().view(np.uint32),
            d_counts.cpu().numpy().view(np.uint32).reshape(n, keep), d_strand.cpu().numpy())


@pytest.mark.parametrize("strand,orientation", [("forward", "fr"), ("reverse", "fr"), ("both", "fr"), ("both", "ff")])
def test_device_entry_host_entry_pieces_and_chunks_give_the_same_bytes(placer_cls, small_case, kernel, monkeypatch, strand,
                                                                       orientation):
    import torch
    _, db = small_case
    pairs = _pairs(db.kmer_size, np.random.default_rng(4))
    data, offs = _pack(pairs)
    longest = max(len(a) + len(b) + 1 for a, b in pairs)
    assert longest == 301
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        host = pl.place_mates(data, offs, strand, orientation)
        pl.choose_counts(longest)
        device = _device_run(pl, data, offs, strand, orientation, stream, guard=4096)
        pieces = [pl.place_mates(*_pack(pairs[a:b]), strand, orientation) for a, b in ((0, 7), (7, 100), (100, len(pairs)))]
        monkeypatch.setenv("EPIK_AMD_MATES_CHUNK_READS", "5")
        chunked = pl.place_mates(data, offs, strand, orientation)
    rows, n, counts, label = host
    assert capi.ROWS_COUNTS_TOO_NARROW not in n and int(n.max()) <= pl.keep_at_most
    assert _same_bytes(device, host)
    assert _same_bytes([np.concatenate([p[i] for p in pieces]) for i in range(4)], host)
    assert _same_bytes(chunked, host)
    # row slots past n_rows come back zero
    past = np.arange(rows.shape[1])[None, :] >= n[:, None]
    assert past.any()
    assert not np.frombuffer(rows[past].tobytes(), dtype=np.uint8).any() and not counts[past].any()


@pytest.mark.parametrize("strand", ["forward", "both"])
def test_host_entry_widens_forced_counts_and_restores_them(placer_cls, oracle_lib, small_case, monkeypatch, strand):
    """2 x 150 bp is a sequence of 301 characters: 8-bit counts do not hold its k-mers.  The host entry widens a forced
    width for the call and gives it back; the device entry, with the forced width, marks the pair."""
    import torch
    _, db = small_case
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", "2")     # 8-bit counts (255 k-mers)
    rng = np.random.default_rng(22)
    pairs = [("ACGTACGTAC", "GGTTACGT"), tuple("".join(rng.choice(list("ACGT"), size=150)) for _ in range(2)),
             ("ACGTTGCA" * 4, "TTGACCAA")]
    data, offs = _pack(pairs)
    orc = oracle_lib.Oracle.from_synth(db)
    joined = _joined(pairs)
    fwd, rev = _oracle(orc, joined), _oracle(orc, [rc(j) for j in joined])
    want = {"forward": fwd, "both": both_rule(fwd, rev)[0]}[strand]
    with placer_cls.from_synth(db) as pl:
        got = pl.place_mates(data, offs, strand)
        assert int(got[1].max()) <= pl.keep_at_most and capi.ROWS_COUNTS_TOO_NARROW not in got[1]
        _, dev_n, _, _ = _device_run(pl, data, offs, strand, "fr", torch.cuda.Stream())
    assert_rows_match(*got[:3], *want)
    assert dev_n[1] == capi.ROWS_COUNTS_TOO_NARROW and dev_n[0] != capi.ROWS_COUNTS_TOO_NARROW


def test_workspace_and_mode_checks(placer_cls, small_case, monkeypatch):
    import torch
    select_kernel(monkeypatch, "packed")
    _, db = small_case
    pairs = _pairs(db.kmer_size, np.random.default_rng(5), 50)
    data, offs = _pack(pairs)
    n, seq_bytes = len(pairs), int(offs[-1])
    stream = torch.cuda.Stream()
    with placer_cls.from_synth(db) as pl:
        sizes = {s: pl.mates_workspace_bytes(n, seq_bytes, s) for s in ("forward", "reverse", "both")}
        # the joined bytes and their offsets even in forward; the strand placement's workspace on top
        assert sizes["forward"] >= seq_bytes + n + 8 * (n + 1)
        assert sizes["both"] > sizes["reverse"] >= sizes["forward"] + seq_bytes + n
        assert pl.mates_workspace_bytes(n, seq_bytes, "both", "ff") == sizes["both"]
        assert pl.mates_workspace_bytes(0, 0, "both") == 0
        pl.choose_counts(301)
        for strand in sizes:
            with pytest.raises(capi.EpikAmdError) as e:       # one byte too small
                _device_run(pl, data, offs, strand, "fr", stream, ws_bytes=sizes[strand] - 1)
            assert e.value.code == capi.ERR_INVALID and "workspace smaller" in str(e.value)
        for mode in (3, 0x200, 0x100 | 3, 1 << 31):           # unknown strand modes and bits
            out = __import__("ctypes").c_uint64(5)
            assert pl._lib.epik_amd_placer_mates_workspace_bytes(pl._handle, n, seq_bytes, mode,
                                                                 __import__("ctypes").byref(out)) == capi.ERR_INVALID
            assert out.value == 0
        with pytest.raises(ValueError):
            pl.place_mates(data, offs, "both", "rf")
        with pytest.raises(ValueError):
            pl.place_mates(data, offs[:-1], "both")           # an odd number of reads
        got = pl.place_mates(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert all(len(x) == 0 for x in got)
    amino = synth.make_db(60, states="amino", kmer_size=3, seed=8, p_present=0.3)
    with placer_cls.from_synth(amino) as pl:
        for call in (lambda: pl.place_mates(data, offs), lambda: pl.mates_workspace_bytes(1, 14), pl.mates_separator):
            with pytest.raises(capi.EpikAmdError) as e:
                call()
            assert e.value.code == capi.ERR_UNSUPPORTED


def test_clade_fragments_rows_are_the_oracles_on_the_joined_sequences(placer_cls, oracle_lib, kernel):
    """The case of test_mates_cpu on the GPU: the rows of the pairs are the oracle's rows of J, so the pair finds the whole
    fragment's branch as often as the oracle says (0.839 against 0.721 / 0.729 for either mate alone)."""
    db, refs, _ = synth.make_clade_db(999, n_refs=80, ref_length=700, seed=5)
    data, offs = synth.make_clade_reads(refs, 1000, 400, seed=6)
    flipped = np.arange(1000) % 2 == 1
    fragments = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(1000)]
    fragments = [rc(f) if flip else f for f, flip in zip(fragments, flipped)]
    pairs = [(f[:60], rc(f[-60:])) for f in fragments]
    orc = oracle_lib.Oracle.from_synth(db)
    joined = _joined(pairs)
    want, want_strand = both_rule(_oracle(orc, joined), _oracle(orc, [rc(j) for j in joined]))
    whole = both_rule(_oracle(orc, fragments), _oracle(orc, [rc(f) for f in fragments]))[0][0]["branch"][:, 0]
    with placer_cls.from_synth(db) as pl:
        rows, n, counts, strand = pl.place_mates(*_pack(pairs), "both")
        singles = [pl.place_strands(*synth.pack_reads(m), "both")[0]["branch"][:, 0] for m in zip(*pairs)]
    assert_rows_match(rows, n, counts, *want)
    assert np.array_equal(strand, want_strand) and np.array_equal(strand, flipped)
    share = float((rows["branch"][:, 0] == whole).mean())
    alone = [float((s == whole).mean()) for s in singles]
    print(f"pair {share:.3f}, mates alone {alone[0]:.3f} / {alone[1]:.3f}")
    assert share > max(alone)


def test_profile_mates_equals_the_rule_on_the_placed_rows(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "paired")
    _, db = small_case
    rng = np.random.default_rng(31)
    pairs = _pairs(db.kmer_size, rng, 1200)
    weights = rng.integers(0, 9, size=len(pairs)).astype(np.uint32)
    data, offs = _pack(pairs)
    with placer_cls.from_synth(db) as pl, pl.profile() as profile:
        for strand, orientation in ((None, "fr"), ("both", "fr"), ("reverse", "ff")):
            rows, n_rows, counts, labels = pl.place_mates(data, offs, strand or "forward", orientation)
            want = numpy_rule(rows, n_rows, counts, weights, db.num_branches)
            assert want[2]["placed"] > 0 and want[2]["too_short"] > 0 and want[2]["no_hit"] > 0
            profile.reset()
            got_labels = pl.profile_packed(profile, data, offs, weights, strand=strand, mates=orientation)
            assert_profile(profile.read(), want, f"profile_mates {strand} {orientation}")
            assert np.array_equal(got_labels, labels)
            monkeypatch.setenv("EPIK_AMD_MATES_CHUNK_READS", "5")     # chunks of five pairs
            small = slice(0, 333)
            profile.reset()
            got_labels = pl.profile_packed(profile, *_pack(pairs[small]), weights[small], strand=strand, mates=orientation)
            monkeypatch.delenv("EPIK_AMD_MATES_CHUNK_READS")
            assert_profile(profile.read(), numpy_rule(rows[small], n_rows[small], counts[small], weights[small], db.num_branches),
                           f"chunks of 5 {strand} {orientation}")
            assert np.array_equal(got_labels, labels[small])
        # unweighted: a fragment counts once -- pairs, not mates
        profile.reset()
        pl.profile_packed(profile, data, offs, mates="fr")
        totals = profile.read().totals
        assert totals["placed"] + totals["no_hit"] + totals["too_short"] + totals["too_narrow"] == len(pairs)
        with pytest.raises(ValueError):
            pl.profile_packed(profile, data, offs, mates="fr", translate="both")


def test_place_takes_the_mates_and_merges_equal_pairs(placer_cls, small_case, monkeypatch):
    select_kernel(monkeypatch, "packed")
    tree, db = small_case
    a, b, c = "ACGTTGCAAGGCTTACGATCGGA", "TTGACCATGCAGGAT", "GGATCCATTGACA"
    first = [("p0/1", a), ("p1/1", a), ("p2/1 lane 3", a), ("p3", c)]
    second = [("p0/2", b), ("p1/2", c), ("p2/2", b), ("p3", "")]
    with placer_cls.from_synth(db, tree) as pl, pl.profile() as profile:
        out = pl.place(first, mates=second, strand="both", profile=profile)
        joined = pl.place([("j", mates.join(a, b))], strand="both")
        totals = profile.read().totals
        with pytest.raises(ValueError, match="record 2 of the mates is 'x'"):
            pl.place(first, mates=[second[0], ("x/2", c)] + second[2:])
        with pytest.raises(ValueError, match="no mate for record 4"):
            pl.place(first, mates=second[:3])
    assert out.sequence_map == {(a, b): ["p0/1", "p2/1 lane 3"], (a, c): ["p1/1"], (c, ""): ["p3"]}   # by the PAIR
    assert [(p.sequence, p.mate) for p in out.placed_seqs] == [(a, b), (a, c), (c, "")]
    assert out.placed_seqs[0].placements == joined.placed_seqs[0].placements
    assert out.placed_seqs[0].strand == joined.placed_seqs[0].strand
    assert sum(totals[k] for k in ("placed", "no_hit", "too_short")) == 4


def _write_fasta(path, records):
    with open(path, "w") as fh:
        for h, s in records:
            fh.write(f">{h}\n")
            for j in range(0, len(s), 70):
                fh.write(s[j:j + 70] + "\n")


def test_driver_places_one_fragment_per_pair_end_to_end(placer_cls, tmp_path):
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree = synth.make_tree(500, seed=13)
    db, refs, _ = synth.make_clade_db(tree.num_nodes, n_refs=80, ref_length=700, seed=14)
    db_path = str(tmp_path / "db.ekdb")
    dbfile.write_db(db_path, db, tree.newick())
    data, offs = synth.make_clade_reads(refs, 2500, 300, seed=15)
    fragments = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(2500)]
    flipped = [i % 2 == 1 for i in range(2500)]
    fragments = [rc(f) if flip else f for f, flip in zip(fragments, flipped)]
    pairs = [(f[:100], rc(f[-100:])) for f in fragments]
    # equal pairs and an equal mate 1, in the batch of their twins (the drivers de-duplicate per batch, place.cpp:207)
    pairs += [pairs[2490], pairs[2491], (pairs[2490][0], pairs[2499][1]), ("ACG", "AC"), ("ACGTACGTACGT", "")]
    flipped += [flipped[2490], flipped[2491], None, None, None]
    names = [f"frag_{i}" for i in range(len(pairs))]
    first = [(f"{h}/1 lane=1", a) for h, (a, _) in zip(names, pairs)]
    second = [(f"{h}/2", b) for h, (_, b) in zip(names, pairs)]
    r1, r2 = str(tmp_path / "sample.fasta"), str(tmp_path / "sample_r2.fasta")
    _write_fasta(r1, first)
    _write_fasta(r2, second)
    batch = 777
    assert 2490 // batch == (len(pairs) - 1) // batch
    with placer_cls.from_synth(db, tree) as pl:
        want = [pl.place(first[at:at + batch], mates=second[at:at + batch], strand="both") for at in range(0, len(pairs), batch)]
    unique = sum(len(set(pairs[at:at + batch])) for at in range(0, len(pairs), batch))     # by the PAIR, per batch
    assert sum(len(w.placed_seqs) for w in want) == unique <= len(pairs) - 2
    assert unique > sum(len({a for a, _ in pairs[at:at + batch]}) for at in range(0, len(pairs), batch))
    ref_path = str(tmp_path / "ref.jplace")
    jplace.write_jplace(ref_path, want, "Placer.place(mates=)", tree.newick(jplace=True))
    driver = os.path.join(ROOT, "epik_amd", "bin", "epik-dna")
    runs = {"launcher": None, "profile_j1": ["--profile", "-j", "1"], "profile_j16": ["--profile", "-j", "16"],
            "only_j1": ["--profile-only", "-j", "1"], "only_j16": ["--profile-only", "-j", "16"],
            "only_two_handles": ["--profile-only", "--devices", "0,0", "-j", "4"]}
    outs = {}
    for name, extra in runs.items():
        outs[name] = tmp_path / name
        outs[name].mkdir()
        if extra is None:
            cmd = [sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", db_path, "-o", str(outs[name]), "--strand", "both",
                   "--mates", r2, r1]
        else:
            cmd = [driver, "-d", db_path, "-q", r1, "-o", str(outs[name]), "--batch-size", str(batch), "--strand", "both",
                   "--mates", r2] + extra
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, name + run.stdout[-2000:] + run.stderr[-2000:]
        assert f"Placed {len(pairs)} sequences." in run.stdout
    # one pquery per unique pair, named by mate 1's headers; the rows of Placer.place(mates=)
    got = jplace.read_jplace(str(outs["profile_j1"] / "placements_sample.fasta.jplace"))
    ref = jplace.read_jplace(ref_path)
    assert set(got) == set(ref) == {h for h, _ in first}
    assert jplace_diff.diff_strict(got, ref) == []
    assert got[first[-2][0]] == [] and len(got[first[-1][0]]) > 0
    # the two jplace files of the driver are the same bytes, but for the line that quotes the command line
    a = (outs["profile_j1"] / "placements_sample.fasta.jplace").read_bytes().split(b"\n")
    b = (outs["profile_j16"] / "placements_sample.fasta.jplace").read_bytes().split(b"\n")
    quoted = [i for i, line in enumerate(a) if b'"invocation"' in line]
    assert len(quoted) == 1 and b"--mates" in a[quoted[0]]
    del a[quoted[0]], b[quoted[0]]
    assert a == b and len(a) > 2000
    # the fragment's strand, one line per record of the query, input order
    with open(outs["profile_j1"] / "strands_sample.fasta.tsv") as fh:
        lines = [line.rstrip("\n").split("\t") for line in fh]
    assert [h for h, _ in lines] == [h for h, _ in first]
    marks = np.array([m == "-" for _, m in lines[:2500]])
    assert (marks == np.array(flipped[:2500])).mean() >= 0.99
    for name in outs:
        if name != "launcher":
            assert (outs[name] / "strands_sample.fasta.tsv").read_bytes() == (outs["profile_j1"] / "strands_sample.fasta.tsv").read_bytes()
    # the profile counts fragments, and is the same file with and without the jplace, whatever the threads and handles
    tsv = {name: (path / "profile_sample.fasta.tsv") for name, path in outs.items() if name != "launcher"}
    for name in tsv:
        assert tsv[name].read_bytes() == tsv["profile_j1"].read_bytes(), name
        assert (outs[name] / "placements_sample.fasta.jplace").exists() == name.startswith("profile")
    from epik_amd import profile as profile_mod
    back = profile_mod.read_tsv(str(tsv["only_j16"]))
    assert back["records"] == back["placed"] + back["no_hit"] + back["too_short"] == len(pairs)
    assert back["too_short"] == 1 and back["placed"] >= 2500
    # mates that do not follow the query: named errors
    short, renamed = str(tmp_path / "short_r2.fasta"), str(tmp_path / "renamed_r2.fasta")
    _write_fasta(short, second[:-1])
    _write_fasta(renamed, second[:1000] + [("other/2", second[1000][1])] + second[1001:])
    for r2_bad, message in ((short, f"--mates: the mates end after {len(pairs) - 1} records: no mate for record {len(pairs)} "
                                    f"('{names[-1]}')"),
                            (renamed, f"--mates: record 1001 of the mates is 'other', of the query '{names[1000]}'")):
        bad = tmp_path / ("bad_" + os.path.basename(r2_bad))
        bad.mkdir()
        run = subprocess.run([driver, "-d", db_path, "-q", r1, "-o", str(bad), "--batch-size", str(batch), "--mates", r2_bad],
                             capture_output=True, text=True, timeout=600)
        assert run.returncode == 255, run.stdout[-2000:] + run.stderr[-2000:]
        assert run.stderr.startswith("Error:") and message in run.stderr, run.stderr
