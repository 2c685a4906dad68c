"""Paired-end placement without a GPU: the C ABI's mates entry points exist and refuse a NULL handle; the rule
J = m1 . sep . rc(m2) restated in Python against hand-written cases, and rc(J(m1, m2)) = J(m2, m1) on classes; the
launcher and the driver pass and check --mates; and, on the CPU oracle alone, what joining the mates buys."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import alphabet, mates, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")


def test_mates_symbols_refuse_a_null_handle():
    from epik_amd import capi
    lib = capi.load()
    for name in ("epik_amd_placer_mates_separator", "epik_amd_placer_mates_workspace_bytes",
                 "epik_amd_placer_place_mates_device", "epik_amd_placer_place_mates", "epik_amd_placer_profile_mates"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    out, sep = ctypes.c_uint64(7), ctypes.c_uint8(9)
    assert lib.epik_amd_placer_mates_separator(None, ctypes.byref(sep)) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    assert lib.epik_amd_placer_mates_workspace_bytes(None, 10, 100, capi.STRAND_BOTH, ctypes.byref(out)) == capi.ERR_INVALID
    assert out.value == 0 and b"null placer" in lib.epik_amd_last_error()
    assert lib.epik_amd_placer_place_mates_device(None, None, None, 1, 10, capi.STRAND_BOTH | capi.MATES_FF, None, 0, None,
                                                  None, None, None, None) == capi.ERR_INVALID
    assert lib.epik_amd_placer_place_mates(None, None, None, 1, capi.STRAND_REVERSE, None, None, None,
                                           None) == capi.ERR_INVALID
    assert lib.epik_amd_placer_profile_mates(None, None, None, None, None, 1, capi.STRAND_FORWARD, None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    assert (capi.STRAND_FORWARD, capi.STRAND_REVERSE, capi.STRAND_BOTH, capi.MATES_FF) == (0, 1, 2, 0x100)
    assert capi.MATE_ORIENTATIONS == {"fr": 0, "ff": 0x100}


@pytest.mark.parametrize("m1,m2,fr,ff", [
    ("ACGT", "AACC", "ACGT-GGTT", "ACGT-AACC"),
    ("", "AACC", "-GGTT", "-AACC"),                       # an empty mate on either side
    ("ACGT", "", "ACGT-", "ACGT-"),
    ("", "", "-", "-"),
    ("ACRYKM", "BVDHSWN", "ACRYKM-NWSDHBV", "ACRYKM-BVDHSWN"),   # IUPAC letters
    ("acgt", "aacgn", "acgt-ncgtt", "acgt-aacgn"),        # lower case stays lower case
    ("ACGU", "UUGA", "ACGU-TCAA", "ACGU-UUGA"),           # U complements to A
    ("AC-GT", "A-C", "AC-GT-G-T", "AC-GT-A-C"),           # '-' inside a mate stays where it is
    ("AC*GT", "A.CX", "AC*GT-XG.T", "AC*GT-A.CX"),        # other invalid characters as they are
])
def test_join_against_hand_written_cases(m1, m2, fr, ff):
    assert mates.join(m1, m2) == mates.join(m1, m2, "fr") == fr
    assert mates.join(m1, m2, "ff") == ff
    with pytest.raises(ValueError):
        mates.join(m1, m2, "rf")


def test_separator_is_invalid_in_the_nucleotide_table():
    table = alphabet.char_class_table("nucl")
    assert int(table[ord("-")]) == 0


def test_reverse_strand_of_a_pair_is_the_pair_swapped():
    """rc(m1 . sep . rc(m2)) = m2 . sep . rc(m1), compared on character classes (U comes back as A, same class)."""
    table = alphabet.char_class_table("nucl")
    rng = np.random.default_rng(11)
    letters = list("ACGTUacgtuRYKMBVDHSWNrykmbvdhswn-.*X")

    def classes(read):
        return [int(table[ord(c)]) for c in read]

    for _ in range(300):
        m1 = "".join(rng.choice(letters, size=int(rng.integers(0, 70))))
        m2 = "".join(rng.choice(letters, size=int(rng.integers(0, 70))))
        assert classes(mates.reverse_complement(mates.join(m1, m2))) == classes(mates.join(m2, m1))
        # FF: the reverse strand is the reverse complements of the mates, swapped
        assert classes(mates.reverse_complement(mates.join(m1, m2, "ff"))) == classes(
            mates.join(mates.reverse_complement(m2), mates.reverse_complement(m1), "ff"))
        assert len(mates.join(m1, m2)) == len(m1) + len(m2) + 1


def test_interleave_and_mate_names():
    data, offs = mates.interleave(["ACG", "", "T"], ["TT", "G", ""])
    assert bytes(data) == b"ACGTTGT" and offs.tolist() == [0, 3, 5, 5, 6, 7, 7] and offs.dtype == np.uint64
    assert mates.mate_name("read_7/1 lane=3") == mates.mate_name("read_7/2") == mates.mate_name("read_7\tx") == "read_7"
    assert mates.mate_name("a/3") == "a/3"
    mates.check_mate_names(["a/1", "b extra"], ["a/2", "b"])
    with pytest.raises(ValueError, match=r"record 2 of the mates is 'c', of the query 'b'"):
        mates.check_mate_names(["a", "b"], ["a", "c"])
    with pytest.raises(ValueError, match=r"the mates end after 1 records: no mate for record 2 \('b'\)"):
        mates.check_mate_names(["a", "b"], ["a"])
    with pytest.raises(ValueError, match=r"the query end after 1 records"):
        mates.check_mate_names(["a"], ["a", "b"])


def test_launcher_passes_mates_only_when_given():
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert epik.driver_command(**kw, mates=None, mate_orientation="fr") == default
    assert epik.driver_command(**kw, mate_orientation="ff") == default   # (no mates: nothing to orient)
    assert "--mates" not in default and "--mate-orientation" not in default
    paired = epik.driver_command(**kw, mates="r2.fasta")
    assert paired[:-1] == default[:-1] + ["--mates", "r2.fasta"] and paired[-1] == default[-1]
    ff = epik.driver_command(**kw, mates="r2.fasta", mate_orientation="ff", strand="both")
    assert ff[:-1] == default[:-1] + ["--strand", "both", "--mates", "r2.fasta", "--mate-orientation", "ff"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--mates" in out.stdout and "--mate-orientation" in out.stdout


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("binary,extra,message", [
    ("epik-aa", ["--mates", "r2.fasta"], "--mates places pairs of nucleotide reads only (epik-dna)"),
    ("epik-dna", ["--mates", "r2.fasta", "--translate", "both"], "--mates does not work with --translate"),
    ("epik-dna", ["--mates", "r2.fasta", "--db-shard", "2"], "--mates does not work with --db-shard > 1"),
    ("epik-dna", ["--mates=r2.fasta", "--strand", "both", "--db-shard", "2"], "--db-shard"),
    ("epik-dna", ["--mates", "r2.fasta", "--mate-orientation", "rf"], "--mate-orientation must be fr or ff"),
    ("epik-dna", ["--mate-orientation", "ff"], "--mate-orientation needs --mates"),
])
def test_driver_rejects_mates_before_touching_anything(host_bins, tmp_path, binary, extra, message):
    # (a database, query and mates that do not exist: the error must come before any is opened, or any device asked for)
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.fasta"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and message in run.stderr, run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


def test_driver_help_names_mates(host_bins):
    out = subprocess.run([os.path.join(host_bins, "epik-dna"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--mates" in out.stdout and "--mate-orientation" in out.stdout


def test_joined_mates_find_the_fragments_branch_more_often_than_either_mate(oracle_lib):
    """400 bp fragments of a clade database, every second one reverse-complemented; mates = the first 60 bp and the
    reverse complement of the last 60 bp; everything placed with the `both` strand rule.  The best branch of the whole
    fragment is found strictly more often by the joined pair than by either mate alone (0.839 against 0.721 / 0.729),
    and every fragment's strand comes back right."""
    rc = mates.reverse_complement
    db, refs, _ = synth.make_clade_db(999, n_refs=80, ref_length=700, seed=5)
    data, offs = synth.make_clade_reads(refs, 1000, 400, seed=6)
    flipped = np.arange(1000) % 2 == 1
    fragments = [bytes(data[int(offs[i]):int(offs[i + 1])]).decode() for i in range(1000)]
    fragments = [rc(f) if flip else f for f, flip in zip(fragments, flipped)]
    mate1, mate2 = [f[:60] for f in fragments], [rc(f[-60:]) for f in fragments]
    orc = oracle_lib.Oracle.from_synth(db)

    def best_of_both(reads):
        (fr, fn, _), (rr, rn, _) = (orc.place(*synth.pack_reads(x), num_threads=0) for x in (reads, [rc(r) for r in reads]))
        take = (rn != 0) & ((fn == 0) | (rr["score"][:, 0] > fr["score"][:, 0]))
        return np.where(take, rr["branch"][:, 0], fr["branch"][:, 0]), take

    whole, whole_strand = best_of_both(fragments)
    first, _ = best_of_both(mate1)
    second, _ = best_of_both(mate2)
    joined, strand = best_of_both([mates.join(a, b) for a, b in zip(mate1, mate2)])
    share = {name: float((best == whole).mean()) for name, best in (("mate 1", first), ("mate 2", second), ("pair", joined))}
    print(f"agree with the whole fragment: {share}; the two mates with each other: {float((first == second).mean()):.3f}")
    assert share["pair"] > share["mate 1"] and share["pair"] > share["mate 2"], share
    assert np.array_equal(strand, flipped) and np.array_equal(whole_strand, flipped)
