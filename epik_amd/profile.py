"""The abundance profile of a sample (`epik_amd_profile`, include/epik_amd.h): per branch the summed like-weight
ratios in 2^-30 fixed point (`mass`) and the reads whose best placement is that branch (`best`); per sample how many
reads were placed, had no hit, were too short.  Summed on the device from the rows a placement left there, in
integers: the same bits whatever the batches, the grid or the order.

`Profile` is the ctypes side of the device object; `clade_sums`, `write_tsv` and `read_tsv` are the file the drivers
write with --profile / --profile-only (epik_amd/host/profile.cpp writes the same bytes).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import capi

LWR_BITS = capi.PROFILE_LWR_BITS
TOTALS = ("placed", "no_hit", "too_short", "too_narrow", "bad_rows")
HEADER = "edge_num\tbest\tmass_q\tmass\tclade_best\tclade_mass_q\tclade_mass"


def quantise(lwr) -> np.ndarray:
    """q(x) = llrint(x * 2^30), round half to even."""
    return np.rint(np.asarray(lwr, dtype=np.float64) * float(1 << LWR_BITS)).astype(np.int64).astype(np.uint64)


def clade_sums(per_branch, subtree_num_nodes) -> np.ndarray:
    """Sums over subtrees: with post-order ids the subtree of branch b is the id range
    [b - subtree_num_nodes[b] + 1, b], so the sums are differences of a prefix sum (uint64, wrapping)."""
    per_branch = np.asarray(per_branch, dtype=np.uint64)
    size = np.asarray(subtree_num_nodes, dtype=np.int64)
    ids = np.arange(len(per_branch), dtype=np.int64)
    if len(size) != len(per_branch) or (size < 1).any() or (size > ids + 1).any():
        raise ValueError("subtree_num_nodes does not describe ranges of post-order ids")
    prefix = np.zeros(len(per_branch) + 1, dtype=np.uint64)
    np.cumsum(per_branch, dtype=np.uint64, out=prefix[1:])
    return prefix[ids + 1] - prefix[ids + 1 - size]


@dataclass
class SampleProfile:
    """What a profile holds on the host: `mass` and `best` uint64 [num_branches], `totals` by name."""

    mass: np.ndarray
    best: np.ndarray
    totals: dict = field(default_factory=lambda: dict.fromkeys(TOTALS, 0))

    @property
    def records(self) -> int:
        return sum(int(self.totals[k]) for k in ("placed", "no_hit", "too_short", "too_narrow")) & (2 ** 64 - 1)

    def merged(self, other: "SampleProfile") -> "SampleProfile":
        """The profile of both samples together: integer sums (modulo 2^64)."""
        return SampleProfile(self.mass + other.mass, self.best + other.best,
                             {k: (int(self.totals[k]) + int(other.totals[k])) & (2 ** 64 - 1) for k in TOTALS})


def format_tsv(profile: SampleProfile, subtree_num_nodes) -> str:
    t = profile.totals
    lines = [f"# epik_amd profile v1\tlwr_bits={LWR_BITS}\trecords={profile.records}\tplaced={int(t['placed'])}"
             f"\tno_hit={int(t['no_hit'])}\ttoo_short={int(t['too_short'])}", HEADER]
    clade_best, clade_mass = clade_sums(profile.best, subtree_num_nodes), clade_sums(profile.mass, subtree_num_nodes)
    scale = float(1 << LWR_BITS)
    for b in range(len(profile.mass)):
        m, cm = int(profile.mass[b]), int(clade_mass[b])
        lines.append(f"{b}\t{int(profile.best[b])}\t{m}\t{float(m) / scale:.9f}\t{int(clade_best[b])}\t{cm}\t{float(cm) / scale:.9f}")
    return "\n".join(lines) + "\n"


def write_tsv(path: str, profile: SampleProfile, subtree_num_nodes) -> None:
    """profile_<input>.tsv as epik-dna / epik-aa --profile write it; edge_num is the branch's post-order id, the number
    the jplace carries for it."""
    with open(path, "w", newline="") as fh:
        fh.write(format_tsv(profile, subtree_num_nodes))


def read_tsv(path: str) -> dict:
    """The file back: {"lwr_bits", "records", "placed", "no_hit", "too_short": int; "edge_num", "best", "mass_q",
    "clade_best", "clade_mass_q": uint64 arrays; "mass", "clade_mass": float64 arrays}."""
    with open(path, newline="") as fh:
        first = fh.readline().rstrip("\n").split("\t")
        if first[0] != "# epik_amd profile v1":
            raise ValueError(f"{path}: not an epik_amd profile (v1)")
        out = {k: int(v) for k, v in (item.split("=") for item in first[1:])}
        names = fh.readline().rstrip("\n").split("\t")
        if "\t".join(names) != HEADER:
            raise ValueError(f"{path}: unexpected columns {names}")
        cols = [[] for _ in names]
        for line in fh:
            for col, item in zip(cols, line.rstrip("\n").split("\t")):
                col.append(item)
    for name, col in zip(names, cols):
        out[name] = (np.array(col, dtype=np.float64) if name in ("mass", "clade_mass")
                     else np.array([int(x) for x in col], dtype=np.uint64))
    return out


class Profile:
    """A device profile for one placer (`epik_amd_profile_create`): all zero at first; `add_device` adds the rows a
    placement left in device memory, `read` gives the sums so far.  A context manager; `close()` frees it."""

    def __init__(self, placer):
        self._lib = capi.load()
        self._handle = ctypes.c_void_p()
        capi.check(self._lib.epik_amd_profile_create(placer._handle, ctypes.byref(self._handle)))
        self.device = placer.device
        self.num_branches = placer.num_branches
        self.keep_at_most = placer.keep_at_most

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.epik_amd_profile_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def lds_path(self) -> bool:
        """Whether add_device sums in LDS first (else straight into global memory)."""
        lds = ctypes.c_uint32(0)
        capi.check(self._lib.epik_amd_profile_info(self._handle, None, ctypes.byref(lds)))
        return bool(lds.value)

    def add_device(self, d_rows: int, d_n_rows: int, d_kmer_counts: int, n: int, d_weights: int = 0, stream: int = 0) -> None:
        """Device pointers, asynchronous on `stream` (`epik_amd_profile_add_device`); `d_weights` 0: every read once."""
        capi.check(self._lib.epik_amd_profile_add_device(self._handle, d_rows or None, d_n_rows or None,
                                                         d_kmer_counts or None, d_weights or None, int(n), stream or None))

    def add_host(self, rows: np.ndarray, n_rows: np.ndarray, kmer_counts: np.ndarray, weights=None) -> None:
        """Rows that are in host memory (Placer.place_packed's): copied to the profile's device (through torch) and
        added there."""
        import torch
        dev = torch.device("cuda", self.device)
        n = int(len(n_rows))
        if n == 0:
            return
        rows = np.ascontiguousarray(rows, dtype=capi.PLACEMENT).reshape(n, self.keep_at_most)
        d_rows = torch.from_numpy(rows.view(np.float64).reshape(-1)).to(dev)
        d_n = torch.from_numpy(np.ascontiguousarray(n_rows, dtype=np.uint32).view(np.int32)).to(dev)
        d_counts = torch.from_numpy(np.ascontiguousarray(kmer_counts, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
        d_w = None if weights is None else torch.from_numpy(
            np.ascontiguousarray(weights, dtype=np.uint32).view(np.int32)).to(dev)
        torch.cuda.synchronize(dev)
        self.add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, 0 if d_w is None else d_w.data_ptr())
        torch.cuda.synchronize(dev)

    def read(self) -> SampleProfile:
        """Synchronises the device and returns the sums (`epik_amd_profile_read`)."""
        mass, best = np.zeros(self.num_branches, np.uint64), np.zeros(self.num_branches, np.uint64)
        totals = capi.ProfileTotals()
        capi.check(self._lib.epik_amd_profile_read(self._handle, mass.ctypes.data, best.ctypes.data, ctypes.byref(totals)))
        return SampleProfile(mass, best, {k: int(getattr(totals, k)) for k in TOTALS})

    def reset(self) -> None:
        capi.check(self._lib.epik_amd_profile_reset(self._handle))
