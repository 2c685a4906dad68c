"""Translated placement without a GPU: the library's codon table against one built here from the 64 standard codons
written out letter by letter; the frame lengths; the launcher and the driver pass and check --translate; the C ABI's
frame entry points exist and refuse a NULL handle.  The host-side translation below is what the GPU tests feed the
CPU oracle."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")

# NCBI translation table 1 (the standard code; table 11 translates the same), written out codon by codon
STANDARD_CODE = {
    "TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S",
    "TAT": "Y", "TAC": "Y", "TAA": "*", "TAG": "*", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W",
    "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "CCT": "P", "CCC": "P", "CCA": "P", "CCG": "P",
    "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "CGT": "R", "CGC": "R", "CGA": "R", "CGG": "R",
    "ATT": "I", "ATC": "I", "ATA": "I", "ATG": "M", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T",
    "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R",
    "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A",
    "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G",
}
assert len(STANDARD_CODE) == 64
# the nucleotide class masks of the table's index: A C G T = bits 0 1 2 3; IUPAC codes; U is T
NUCL_BIT = {"A": 1, "C": 2, "G": 4, "T": 8}
IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
         "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "U": "A", "R": "Y", "Y": "R", "K": "M", "M": "K", "S": "S",
              "W": "W", "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
FRAME_NAMES = ("+1", "+2", "+3", "-1", "-2", "-3")


def nucl_class(ch: str) -> int:
    return sum(NUCL_BIT[b] for b in IUPAC.get(ch.upper(), ""))


def residue_of_classes(c0: int, c1: int, c2: int) -> str:
    if not (c0 and c1 and c2):
        return "*"
    bases = [[b for b in "ACGT" if c & NUCL_BIT[b]] for c in (c0, c1, c2)]
    found = {STANDARD_CODE["".join(t)] for t in itertools.product(*bases)}
    amino = found - {"*"}
    if found == {"*"}:
        return "*"
    if "*" in found:
        return "X"
    if len(amino) == 1:
        return amino.pop()
    return {frozenset("DN"): "B", frozenset("EQ"): "Z", frozenset("IL"): "J"}.get(frozenset(amino), "X")


def python_codon_table() -> np.ndarray:
    return np.array([ord(residue_of_classes(i >> 8 & 15, i >> 4 & 15, i & 15)) for i in range(4096)], dtype=np.uint8)


def revcomp(read: str) -> str:
    return "".join(COMPLEMENT.get(c.upper(), "-") if nucl_class(c) else c for c in reversed(read))


def translate(read: str) -> str:
    """Codons from offset 0, the incomplete trailing one dropped."""
    return "".join(residue_of_classes(*(nucl_class(c) for c in read[j:j + 3])) for j in range(0, len(read) - 2, 3))


def frames(read: str, mode: str) -> list:
    """The frames of `mode` in the library's order (+1 +2 +3 -1 -2 -3)."""
    out = []
    if mode in ("forward", "both"):
        out += [translate(read[f:]) for f in range(3)]
    if mode in ("reverse", "both"):
        rc = revcomp(read)
        out += [translate(rc[f:]) for f in range(3)]
    return out


def frame_length(L: int, f: int) -> int:
    return max((L - f + 1) // 3, 0)


def test_codon_table_equals_the_standard_code():
    from epik_amd.placer import Placer
    got = Placer.codon_table()
    want = python_codon_table()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(i), chr(got[i]), chr(want[i])) for i in bad[:10]]
    # a few written out
    idx = lambda s: nucl_class(s[0]) << 8 | nucl_class(s[1]) << 4 | nucl_class(s[2])
    for codon, aa in (("ATG", "M"), ("TAA", "*"), ("TRA", "*"), ("GAY", "D"), ("RAY", "B"), ("SAR", "Z"),
                      ("MTH", "J"), ("TAN", "X"), ("NNN", "X"), ("GCN", "A"), ("A-G", "*"), ("aug", "M"),
                      ("YTR", "L"), ("MGR", "R"), ("TGR", "X")):
        assert chr(got[idx(codon)]) == aa, codon
    # every plain codon
    for codon, aa in STANDARD_CODE.items():
        assert chr(got[idx(codon)]) == aa


@pytest.mark.parametrize("L", range(11))
def test_frame_lengths(L):
    rng = np.random.default_rng(L)
    read = "".join(rng.choice(list("ACGTN"), size=L))
    fr = frames(read, "both")
    for f in (1, 2, 3):
        assert len(fr[f - 1]) == len(fr[f + 2]) == frame_length(L, f)
    # one direction's three frames hold max(L - 2, 0) residues: the per-read total the library scans
    assert sum(len(x) for x in fr[:3]) == max(L - 2, 0)


def test_reverse_frames_are_the_reverse_complement_translated():
    read = "ATGAAACCCGGGTTTTAG"
    assert frames(read, "forward")[0] == "MKPGF*"
    assert revcomp(read) == "CTAAAACCCGGGTTTCAT"
    assert frames(read, "reverse") == [translate("CTAAAACCCGGGTTTCAT"), translate("TAAAACCCGGGTTTCAT"),
                                       translate("AAAACCCGGGTTTCAT")]


def test_launcher_passes_translate_only_when_given():
    import epik
    kw = dict(database="db.ekdb", states="amino", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert epik.driver_command(**kw, translate=None) == default
    assert "--translate" not in default
    for mode in ("forward", "reverse", "both"):
        argv = epik.driver_command(**kw, translate=mode)
        assert argv[:-1] == default[:-1] + ["--translate", mode] and argv[-1] == default[-1]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True,
                         text=True)
    assert out.returncode == 0 and "--translate" in out.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", __file__, "-o", ROOT,
                          "--translate", "sideways", __file__], capture_output=True, text=True)
    assert bad.returncode != 0 and "--translate" in bad.stderr


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


@pytest.mark.parametrize("binary,extra,message", [
    ("epik-aa", ["--translate", "sideways"], "--translate must be forward, reverse or both"),
    ("epik-dna", ["--translate", "both"], "amino-acid databases only"),
    ("epik-dna", ["--translate=forward"], "amino-acid databases only"),
    ("epik-aa", ["--translate", "both", "--db-shard", "2"], "--db-shard"),
    ("epik-aa", ["--translate=reverse", "--db-shard", "3"], "--db-shard"),
])
def test_driver_rejects_translate_before_touching_anything(host_bins, tmp_path, binary, extra, message):
    # (a database and query that do not exist: the error must come before either is opened, or any device asked for)
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.fasta"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and message in run.stderr, run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


def test_driver_help_names_translate(host_bins):
    out = subprocess.run([os.path.join(host_bins, "epik-aa"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--translate" in out.stdout


def test_frame_symbols_refuse_a_null_handle():
    from epik_amd import capi
    lib = capi.load()
    for name in ("epik_amd_codon_table", "epik_amd_placer_frame_workspace_bytes",
                 "epik_amd_placer_place_frames_device", "epik_amd_placer_place_frames"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    out = ctypes.c_uint64(7)
    assert lib.epik_amd_placer_frame_workspace_bytes(None, 10, 100, capi.FRAMES_BOTH, ctypes.byref(out)) == capi.ERR_INVALID
    assert out.value == 0
    assert lib.epik_amd_placer_place_frames_device(None, None, None, 1, capi.FRAMES_BOTH, None, 0, None, None, None,
                                                   None, None) == capi.ERR_INVALID
    assert lib.epik_amd_placer_place_frames(None, None, None, 1, capi.FRAMES_REVERSE, None, None, None,
                                            None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    assert lib.epik_amd_codon_table(None) == capi.ERR_INVALID
    assert (capi.FRAMES_FORWARD, capi.FRAMES_REVERSE, capi.FRAMES_BOTH) == (0, 1, 2)
    assert capi.FRAME_NAMES == FRAME_NAMES
