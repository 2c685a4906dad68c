"""Strand placement without a GPU: the complement the library takes on character classes (a 4-bit reversal of the
class bitmask) is the IUPAC complement on the nucleotide table; the launcher and the driver pass and check --strand;
the C ABI's strand entry points exist and refuse a NULL handle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from epik_amd import alphabet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")

# the IUPAC complement, written out letter by letter (not derived from the class table)
IUPAC_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "K": "M", "M": "K",
                    "S": "S", "W": "W", "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}


def comp(c: int) -> int:
    ch = chr(c)
    if ch.upper() in IUPAC_COMPLEMENT:
        out = IUPAC_COMPLEMENT[ch.upper()]
        return ord(out.lower() if ch.islower() else out)
    return c


def rc(read: bytes) -> bytes:
    return bytes(comp(c) for c in reversed(read))


def bitrev4(x: int) -> int:
    return int(f"{x:04b}"[::-1], 2)


def test_complement_is_the_bit_reversal_of_the_class():
    table = alphabet.char_class_table("nucl")
    assert alphabet.NUCL_STATES == "ACGT"   # (state s <-> 3 - s is the complement only in this order)
    for c in range(256):
        assert int(table[comp(c)]) == bitrev4(int(table[c])), (chr(c), int(table[c]), int(table[comp(c)]))
    # the classes the issue names
    for a, b in (("R", "Y"), ("K", "M"), ("B", "V"), ("D", "H"), ("S", "S"), ("W", "W"), ("N", "N"), ("U", "A")):
        assert bitrev4(int(table[ord(a)])) == int(table[ord(b)])
    assert bitrev4(int(table[ord("-")])) == 0 == int(table[ord("-")])


def test_reverse_complement_twice_keeps_the_class_sequence():
    table = alphabet.char_class_table("nucl")
    rng = np.random.default_rng(3)
    letters = list(b"ACGTUacgtuRYKMBVDHSWNrykmbvdhswn-.*X")
    for _ in range(200):
        read = bytes(rng.choice(letters, size=int(rng.integers(0, 90))).tolist())
        twice = rc(rc(read))
        assert [int(table[c]) for c in twice] == [int(table[c]) for c in read]
        # and the reverse strand's classes are the reversed, bit-reversed classes of the read
        assert [int(table[c]) for c in rc(read)] == [bitrev4(int(table[c])) for c in reversed(read)]


def test_launcher_passes_strand_only_when_not_forward():
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert epik.driver_command(**kw, strand="forward") == default
    assert "--strand" not in default
    both = epik.driver_command(**kw, strand="both")
    assert both[:-1] == default[:-1] + ["--strand", "both"] and both[-1] == default[-1]
    out = subprocess.run([__import__("sys").executable, os.path.join(ROOT, "epik.py"), "place", "--help"],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "--strand" in out.stdout


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("binary,extra,message", [
    ("epik-dna", ["--strand", "sideways"], "--strand must be forward, reverse or both"),
    ("epik-aa", ["--strand", "both"], "nucleotide"),
    ("epik-dna", ["--strand", "both", "--db-shard", "2"], "--db-shard"),
    ("epik-dna", ["--strand=reverse", "--db-shard", "2"], "--db-shard"),
])
def test_driver_rejects_strand_before_touching_anything(host_bins, tmp_path, binary, extra, message):
    # (a database and query that do not exist: the error must come before either is opened, or any device asked for)
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.fasta"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and message in run.stderr, run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


def test_driver_help_names_strand(host_bins):
    out = subprocess.run([os.path.join(host_bins, "epik-dna"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--strand" in out.stdout


def test_strand_symbols_refuse_a_null_handle():
    from epik_amd import capi
    lib = capi.load()
    for name in ("epik_amd_placer_strand_workspace_bytes", "epik_amd_placer_place_strands_device",
                 "epik_amd_placer_place_strands"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    out = ctypes.c_uint64(7)
    assert lib.epik_amd_placer_strand_workspace_bytes(None, 10, 100, capi.STRAND_BOTH, ctypes.byref(out)) == capi.ERR_INVALID
    assert lib.epik_amd_placer_place_strands_device(None, None, None, 1, capi.STRAND_BOTH, None, 0, None, None, None,
                                                    None, None) == capi.ERR_INVALID
    assert lib.epik_amd_placer_place_strands(None, None, None, 1, capi.STRAND_REVERSE, None, None, None,
                                             None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    assert (capi.STRAND_FORWARD, capi.STRAND_REVERSE, capi.STRAND_BOTH) == (0, 1, 2)
