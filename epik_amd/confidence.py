"""Per-read placement confidence (`epik_amd_tree`, `epik_amd_confidence`, include/epik_amd.h): for every read the LCA
clade that holds a share tau of its placement mass, that clade's mass, and the EDPL -- computed on the device from the
rows a placement left there, by one rule that the kernel, the host mirror (epik_amd/host/confidence.cpp) and the tests'
numpy follow to the bit.

`Tree` is the ctypes side of the device object, `HostTables` the same tables in host memory (no device: the LCA query the
kernel runs, for CPU tests); `tau_q`, `clade_counts`, `format_assign_tsv` / `format_clades_tsv` and the readers are the
two files the drivers write with --assign (epik_amd/host/confidence.cpp writes the same bytes).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .profile import clade_sums

LWR_BITS = capi.PROFILE_LWR_BITS
CLASSES = ("too_narrow", "too_short", "no_hit", "bad_row")
CLADES_HEADER = "edge_num\tassigned\tclade_assigned"


def tau_q(tau: float) -> int:
    """--assign-mass as the rule takes it: llrint(tau * 2^30), tau in [0, 1]."""
    tau = float(tau)
    if not 0.0 <= tau <= 1.0:
        raise ValueError(f"the assigned mass must lie in [0, 1], not {tau}")
    return int(np.rint(np.float64(tau) * np.float64(1 << LWR_BITS)))


def parents_of(parent) -> np.ndarray:
    """parent[] as the C ABI takes it: uint32, the root's (-1 in synth.SynthTree) EPIK_AMD_TREE_NO_PARENT."""
    parent = np.asarray(parent).astype(np.int64)
    return np.where(parent < 0, capi.TREE_NO_PARENT, parent).astype(np.uint32)


class HostTables:
    """The tables of a tree in host memory (`epik_amd_tree_build_host`); `lca` is `epik_amd_tree_lca_host`."""

    def __init__(self, parent, branch_length):
        self._lib = capi.load()
        self.parent = np.ascontiguousarray(parents_of(parent))
        self.branch_length = np.ascontiguousarray(branch_length, dtype=np.float64)
        if self.parent.shape != self.branch_length.shape or self.parent.ndim != 1:
            raise ValueError("parent and branch_length must be two arrays of num_branches entries")
        self.num_branches = int(self.parent.shape[0])
        size = ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_tree_build_host(None, None, self.num_branches, None, ctypes.byref(size)))
        self.tables = np.zeros(int(size.value), dtype=np.uint8)
        capi.check(self._lib.epik_amd_tree_build_host(self.parent.ctypes.data, self.branch_length.ctypes.data, self.num_branches,
                                                      self.tables.ctypes.data, ctypes.byref(size)))
        self.table_bytes = int(size.value)

    def lca(self, a, b) -> np.ndarray:
        a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
        out = np.zeros(a.shape, dtype=np.uint32)
        capi.check(self._lib.epik_amd_tree_lca_host(self.tables.ctypes.data, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data))
        return out


class Tree:
    """A tree on a device (`epik_amd_tree_create`), independent of any placer.  A context manager; `close()` frees it."""

    def __init__(self, device: int, parent, branch_length):
        self._lib = capi.load()
        parent = np.ascontiguousarray(parents_of(parent))
        branch_length = np.ascontiguousarray(branch_length, dtype=np.float64)
        if parent.shape != branch_length.shape or parent.ndim != 1:
            raise ValueError("parent and branch_length must be two arrays of num_branches entries")
        self._handle = ctypes.c_void_p()
        capi.check(self._lib.epik_amd_tree_create(int(device), parent.ctypes.data, branch_length.ctypes.data, int(parent.shape[0]),
                                                  ctypes.byref(self._handle)))
        self.device = int(device)
        self.num_branches = int(parent.shape[0])

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.epik_amd_tree_destroy(self._handle)
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

    def info(self) -> dict:
        n, levels, size = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_tree_info(self._handle, ctypes.byref(n), ctypes.byref(levels), ctypes.byref(size)))
        return {"num_branches": int(n.value), "levels": int(levels.value), "table_bytes": int(size.value)}

    def confidence_device(self, d_rows: int, d_n_rows: int, d_kmer_counts: int, n: int, keep: int, tau_q: int, d_out: int,
                          stream: int = 0) -> None:
        """Device pointers, asynchronous on `stream` (`epik_amd_confidence_device`)."""
        capi.check(self._lib.epik_amd_confidence_device(self._handle, d_rows or None, d_n_rows or None, d_kmer_counts or None,
                                                        int(n), int(keep), int(tau_q), d_out or None, stream or None))


def subtree_sizes(parent) -> np.ndarray:
    """size[b] of the rule from parent[] (post-order ids: children come before their parent)."""
    parent = np.asarray(parent).astype(np.int64)
    size = np.ones(len(parent), dtype=np.int64)
    for b in range(len(parent) - 1):
        size[parent[b]] += size[b]
    return size


def clade_counts(conf, weights, num_branches: int):
    """What assign_clades_<input>.tsv holds: assigned[b] = the records whose clade is b (unique sequence i counting
    weights[i] records; None: 1), and the records of each class."""
    conf = np.asarray(conf, dtype=capi.CONFIDENCE)
    w = np.ones(len(conf), np.uint64) if weights is None else np.asarray(weights).astype(np.uint64)
    assigned = np.zeros(num_branches, np.uint64)
    ok = conf["clade"] < np.uint32(num_branches)
    np.add.at(assigned, conf["clade"][ok], w[ok])
    classes = {name: int(w[conf["clade"] == np.uint32(code)].sum(dtype=np.uint64)) for code, name in capi.CLADE_CLASSES.items()}
    return assigned, classes


def format_assign_line(name: str, rec, sizes) -> str:
    clade = int(rec["clade"])
    if clade in capi.CLADE_CLASSES:
        return f"{name}\t{capi.CLADE_CLASSES[clade]}\t0\t{0.0:.9f}\t{0.0:.17g}"
    return (f"{name}\t{clade}\t{int(sizes[clade])}\t{float(int(rec['clade_mass_q'])) / float(1 << LWR_BITS):.9f}"
            f"\t{float(rec['edpl']):.17g}")


def format_assign_tsv(names, conf, sizes, tau_q_value: int) -> str:
    """assign_<input>.tsv: one line per input record, `names[i]` with the record `conf[i]`."""
    lines = [f"# epik_amd assign v1\ttau_q={int(tau_q_value)}\trecords={len(names)}"]
    lines += [format_assign_line(name, rec, sizes) for name, rec in zip(names, conf)]
    return "\n".join(lines) + "\n"


def format_clades_tsv(assigned, classes: dict, sizes, tau_q_value: int) -> str:
    """assign_clades_<input>.tsv: per branch the records assigned to it and to its clade."""
    assigned = np.asarray(assigned, dtype=np.uint64)
    in_clade = clade_sums(assigned, sizes)
    total = int(assigned.sum(dtype=np.uint64))
    records = total + sum(int(classes[k]) for k in CLASSES)
    head = f"# epik_amd assign_clades v1\ttau_q={int(tau_q_value)}\trecords={records}\tassigned_records={total}"
    head += "".join(f"\t{k}={int(classes[k])}" for k in CLASSES)
    lines = [head, CLADES_HEADER] + [f"{b}\t{int(assigned[b])}\t{int(in_clade[b])}" for b in range(len(assigned))]
    return "\n".join(lines) + "\n"


def read_assign_tsv(path: str) -> dict:
    """The file back: {"tau_q", "records": int; "names": list; "edge_num": list of int or class name; "clade_size":
    int64, "clade_mass", "edpl": float64 arrays}."""
    with open(path, newline="") as fh:
        first = fh.readline().rstrip("\n").split("\t")
        if first[0] != "# epik_amd assign v1":
            raise ValueError(f"{path}: not an epik_amd assign file (v1)")
        out = {k: int(v) for k, v in (item.split("=") for item in first[1:])}
        names, edges, sizes, mass, edpl = [], [], [], [], []
        for line in fh:
            name, edge, size, m, e = line.rstrip("\n").rsplit("\t", 4)
            names.append(name), edges.append(edge if edge in CLASSES else int(edge)), sizes.append(int(size))
            mass.append(float(m)), edpl.append(float(e))
    out.update(names=names, edge_num=edges, clade_size=np.array(sizes, np.int64), clade_mass=np.array(mass, np.float64),
               edpl=np.array(edpl, np.float64))
    return out


def read_clades_tsv(path: str) -> dict:
    with open(path, newline="") as fh:
        first = fh.readline().rstrip("\n").split("\t")
        if first[0] != "# epik_amd assign_clades v1":
            raise ValueError(f"{path}: not an epik_amd assign_clades file (v1)")
        out = {k: int(v) for k, v in (item.split("=") for item in first[1:])}
        if fh.readline().rstrip("\n") != CLADES_HEADER:
            raise ValueError(f"{path}: unexpected columns")
        cols = np.array([[int(x) for x in line.split("\t")] for line in fh], dtype=np.uint64).reshape(-1, 3)
    out.update(edge_num=cols[:, 0], assigned=cols[:, 1], clade_assigned=cols[:, 2])
    return out
