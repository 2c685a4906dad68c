"""Paired-end reads on the host: the rule of `epik_amd_placer_place_mates` (include/epik_amd.h) restated in plain
Python, for tests and for callers that want the joined sequence the library places, and the check the drivers make of
a mates file against its query.

    J = m1 . sep . rc(m2)     "fr" (Illumina paired-end)
    J = m1 . sep . m2         "ff"

The placement of a pair is the placement of J; rc(J(m1, m2)) has the classes of J(m2, m1): the reverse strand of a
fragment is the pair with its mates swapped.
"""
from __future__ import annotations

import numpy as np

# the IUPAC complement (U complements to A); any other character stays as it is
_COMPLEMENT = str.maketrans("ACGTUacgtuRYKMBVDHrykmbvdhSWNswn", "TGCAAtgcaaYRMKVBHDyrmkvbhdSWNswn")

ORIENTATIONS = ("fr", "ff")


def reverse_complement(read: str) -> str:
    return read.translate(_COMPLEMENT)[::-1]


def join(mate1: str, mate2: str, orientation: str = "fr", sep: str = "-") -> str:
    """The sequence placed for the pair (mate1, mate2)."""
    if orientation not in ORIENTATIONS:
        raise ValueError(f"unknown mate orientation {orientation!r}: expected one of {list(ORIENTATIONS)}")
    return mate1 + sep + (reverse_complement(mate2) if orientation == "fr" else mate2)


def interleave(mates1, mates2) -> tuple:
    """(seqs uint8, seq_offsets uint64 [2 n + 1]) of the pairs (mates1[i], mates2[i]): read 2 i is mate 1, read 2 i + 1
    mate 2 -- the batch `Placer.place_mates` takes."""
    if len(mates1) != len(mates2):
        raise ValueError("as many first mates as second mates")
    bufs = [m.encode() for pair in zip(mates1, mates2) for m in pair]
    offsets = np.zeros(len(bufs) + 1, dtype=np.uint64)
    if bufs:
        offsets[1:] = np.cumsum([len(b) for b in bufs], dtype=np.uint64)
    return (np.frombuffer(b"".join(bufs), dtype=np.uint8).copy() if bufs else np.zeros(0, np.uint8)), offsets


def mate_name(header: str) -> str:
    """The name two mates share: the header up to the first white space, without a trailing /1 or /2."""
    name = header.split(None, 1)[0] if header.strip() else ""
    return name[:-2] if name.endswith(("/1", "/2")) else name


def check_mate_names(headers, mate_headers) -> None:
    """The records of a mates file follow the query's, one for one, under the same names (epik-dna --mates makes the
    same check, in the same words)."""
    for i, (a, b) in enumerate(zip(headers, mate_headers)):
        if mate_name(a) != mate_name(b):
            raise ValueError(f"record {i + 1} of the mates is '{mate_name(b)}', of the query '{mate_name(a)}': the mates "
                             "must come in the order of the query")
    if len(headers) != len(mate_headers):
        both = min(len(headers), len(mate_headers))
        longer = headers if len(headers) > both else mate_headers
        raise ValueError(f"the {'mates' if len(headers) > both else 'query'} end after {both} records: no mate for record "
                         f"{both + 1} ('{mate_name(longer[both])}')")
