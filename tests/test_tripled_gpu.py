"""The tripled k-mer table on the device (place_device.hpp: kTripledTable): the rows, n_rows and counts of a handle built
with EPIK_AMD_LAYOUT=tripled are bit for bit those of the same handle built with EPIK_AMD_LAYOUT=paired, and agree with
the oracle as tests/test_parity_gpu.py compares.  Small databases, a few thousand reads; the reads aim at where the
lookup takes another form: the tile edge (a phase-2 k-mer on lane 0), an invalid or ambiguous character in front of a
window, reads of one, two and three k-mers."""
import ctypes

import numpy as np
import pytest

from conftest import assert_rows_match, mixed_reads
from epik_amd import capi, synth

pytestmark = pytest.mark.gpu

TABLE_PAIRED, TABLE_TRIPLED = 2, 3


def _reads(k, seed):
    rng = np.random.default_rng(seed)
    plain = lambda n: "".join(rng.choice(list("ACGT"), size=n))  # noqa: E731
    reads = mixed_reads(rng, 1500, k, max_len=200)
    edge = 64 - (k - 1)  # k-mers per 64-character tile: the read of edge + k - 1 characters fills one tile exactly
    for n in (k, k + 1, k + 2, edge - 1, edge, edge + 1, edge + k - 2, edge + k - 1, edge + k, 2 * edge + k, 150, 400):
        reads += [plain(n) for _ in range(40)]
    reads += [plain(n) for n in range(0, k)] + ["", "N" * (k + 3)]
    for t in (0, 1, 5, 17, 18, 19, 30):  # an N at 3t + 1: the k-mer at 3t + 2 is exact, the character in front of it is not
        for at in (3 * t, 3 * t + 1, 3 * t + 2):  # ... and one in each phase, ambiguous (N, R, Y) and invalid (-)
            for ch in "NRY-":
                r = list(plain(150))
                r[at] = ch
                reads.append("".join(r))
    return synth.pack_reads(reads)


CASES = [
    # (leaves, k, EPIK_AMD_WIDE_COUNTS: 0 = u16, 1 = u32, 2 = u8)
    (60, 5, "0"), (60, 5, "1"), (60, 5, "2"),   # N = 119
    (60, 3, "0"), (60, 8, "0"), (60, 8, "1"),
    (500, 5, "0"), (500, 5, "1"),               # N = 999: slack rows
    (600, 5, "0"), (600, 5, "1"),               # N = 1 199: the clamp
]


@pytest.fixture(scope="module")
def references(oracle_lib):
    """The oracle's rows per (leaves, k), computed once."""
    cache = {}

    def get(leaves, k):
        if (leaves, k) not in cache:
            tree = synth.make_tree(leaves, seed=7)
            # (p_present = 0.5: half the codes are absent)
            db = synth.make_db(tree.num_nodes, kmer_size=k, seed=8, p_present=0.5, lognormal=(2.5, 1.5))
            data, offs = _reads(k, seed=leaves + k)
            cache[(leaves, k)] = (db, data, offs, oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0))
        return cache[(leaves, k)]
    return get


def _form(pl):
    out = ctypes.c_uint32(0)
    capi.check(pl._lib.epik_amd_placer_table_form(pl._handle, ctypes.byref(out)))
    return int(out.value)


def _ring(pl, counts):
    out = ctypes.c_uint32(0)
    capi.check(pl._lib.epik_amd_placer_ring_form(pl._handle, counts, ctypes.byref(out)))
    return int(out.value)


@pytest.mark.parametrize("leaves,k,width", CASES)
def test_tripled_rows_are_the_paired_rows_and_the_oracles(gpu_available, references, leaves, k, width, monkeypatch):
    assert gpu_available
    import torch
    from epik_amd.placer import Placer
    db, data, offs, ref = references(leaves, k)
    if width == "2":  # 8-bit counts: the reads of up to 255 k-mers (a longer one in the batch would widen the forced width)
        lengths = np.diff(offs.astype(np.int64))
        short = lengths <= 200
        take = np.concatenate([np.arange(b, b + n) for b, n in zip(offs[:-1][short].astype(np.int64), lengths[short])])
        data = np.ascontiguousarray(data[take])
        offs = np.concatenate([[0], np.cumsum(lengths[short])]).astype(np.uint64)
        ref = tuple(a[short] for a in ref)
    for var in ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_RING_FORM", "EPIK_AMD_MAX_BLOCKS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_WIDE_COUNTS", width)
    dev = torch.device("cuda", 0)
    d_seqs = torch.from_numpy(data).to(dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    torch.cuda.synchronize()
    got = {}
    for layout, form in (("paired", TABLE_PAIRED), ("tripled", TABLE_TRIPLED)):
        monkeypatch.setenv("EPIK_AMD_LAYOUT", layout)
        with Placer.from_synth(db) as pl:
            assert _form(pl) == form
            if layout == "tripled":  # the near ring, with the slack rows where they are free (N = 999)
                assert _ring(pl, 0) == 1 and _ring(pl, 1) & 1
                if leaves != 60:
                    assert _ring(pl, 1) == (3 if leaves == 500 else 1)
            got[layout] = pl.place_packed(data, offs)
            got[layout + "-bytes"] = pl.algorithmic_bytes(d_seqs.data_ptr(), d_offs.data_ptr(), len(offs) - 1)
    (rows_p, n_p, cnt_p), (rows_t, n_t, cnt_t) = got["paired"], got["tripled"]
    assert n_p.tobytes() == n_t.tobytes()
    valid = np.arange(rows_p.shape[1])[None, :] < np.where(n_p == 0xffffffff, 0, n_p)[:, None]
    assert rows_p[valid].tobytes() == rows_t[valid].tobytes() and cnt_p[valid].tobytes() == cnt_t[valid].tobytes()
    assert got["paired-bytes"] == got["tripled-bytes"] > 0
    assert_rows_match(*got["tripled"], *ref)
    assert int(ref[1].sum()) > 1000
