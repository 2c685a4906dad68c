"""Phylo-k-mer databases built from ancestral posteriors (include/epik_amd.h, "Building a phylo-k-mer database").

`Builder` is the device builder (libepik_amd.so: epik_amd_builder_*), `build_host` its host mirror in the library
(epik_amd_build_host), `build_numpy` an independent restatement of the rule in numpy: the three give the same bytes.
`logp_from_posteriors` takes the logarithm as `alphabet.py` does, through libm's log10f.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import alphabet, capi
from .synth import PKDB_VALUE, SynthDB

#: enumeration without pruning up to this many k-mers a window (build_numpy)
UNPRUNED_CODES = 1 << 16

def logp_from_posteriors(p) -> np.ndarray:
    """float32 log10 of posteriors, value by value through log10f (what the placement's threshold goes through);
    p <= 0 gives -inf.  The distinct values are few (a posterior file prints a handful of digits), so each is
    evaluated once."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    uniq, inverse = np.unique(p.reshape(-1), return_inverse=True)
    log10f = alphabet._libm.log10f
    table = np.array([-np.inf if not v > 0 else log10f(ctypes.c_float(float(v))) for v in uniq], dtype=np.float32)
    return table[inverse].reshape(p.shape)


def default_log_thr(states: str, kmer_size: int, omega: float) -> np.float32:
    sigma = alphabet.alphabet_size(states)
    return alphabet.log_threshold(alphabet.score_threshold(omega, kmer_size, sigma))


def _as_db(states, kmer_size, omega, num_branches, log_thr, keys, offsets, values) -> SynthDB:
    db = SynthDB(states=states, kmer_size=int(kmer_size), omega=float(omega), num_branches=int(num_branches),
                 offsets=offsets, values=values, keys=keys)
    db.log_threshold = np.float32(log_thr)
    db.total_entries = int(values.shape[0])
    return db


def _chunk(logp, branch_of, sigma):
    logp = np.ascontiguousarray(logp, dtype=np.float32)
    branch_of = np.ascontiguousarray(branch_of, dtype=np.uint32)
    if logp.ndim != 3 or logp.shape[2] != sigma:
        raise ValueError(f"logp must be [G][L][{sigma}], not {logp.shape}")
    if branch_of.shape != (logp.shape[0],):
        raise ValueError(f"branch_of must be [{logp.shape[0]}], not {branch_of.shape}")
    return logp, branch_of


def _copy_out(lib, handle):
    nk, ne, splits = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    capi.check(lib.epik_amd_builder_finish(handle, ctypes.byref(nk), ctypes.byref(ne), ctypes.byref(splits)))
    keys = np.zeros(nk.value, dtype=np.uint32)
    offsets = np.zeros(nk.value + 1, dtype=np.uint64)
    values = np.zeros(ne.value, dtype=PKDB_VALUE)
    capi.check(lib.epik_amd_builder_copy(handle, keys.ctypes.data, offsets.ctypes.data, values.ctypes.data))
    return keys, offsets, values, int(splits.value)


class Builder:
    """The device builder: chunks of ghost nodes in, a database out.

        with Builder("nucl", 8, tree.num_nodes, omega=1.5) as b:
            b.add(logp, branch_of)          # float32 [G][L][sigma], uint32 [G]
            db = b.finish()                 # SynthDB in the sparse form: Placer.from_synth, dbfile.write_db

    `log_thr` replaces the threshold that follows from omega (tests move it)."""

    def __init__(self, states: str, kmer_size: int, num_branches: int, omega: float = 1.5, log_thr=None, device: int = 0,
                 workspace_bytes: int = 0):
        self._lib = capi.load()
        self.states, self.kmer_size, self.num_branches, self.omega = states, int(kmer_size), int(num_branches), float(omega)
        self.sigma = alphabet.alphabet_size(states)
        self.log_thr = np.float32(default_log_thr(states, kmer_size, omega) if log_thr is None else log_thr)
        self.num_splits = 0
        handle = ctypes.c_void_p()
        capi.check(self._lib.epik_amd_builder_create(int(device), self.sigma, self.kmer_size, self.num_branches,
                                                     ctypes.c_float(float(self.log_thr)), int(workspace_bytes), ctypes.byref(handle)))
        self._handle = handle

    def add(self, logp, branch_of) -> None:
        logp, branch_of = _chunk(logp, branch_of, self.sigma)
        capi.check(self._lib.epik_amd_builder_add(self._handle, logp.ctypes.data, branch_of.ctypes.data, logp.shape[0], logp.shape[1]))

    def add_device(self, d_logp, d_branch_of) -> None:
        """torch tensors on the builder's device: float32 [G][L][sigma] and int32 [G] (the bits of uint32), contiguous."""
        if d_logp.dim() != 3 or d_logp.shape[2] != self.sigma or not d_logp.is_contiguous() or not d_branch_of.is_contiguous():
            raise ValueError(f"logp must be a contiguous [G][L][{self.sigma}] tensor")
        if d_logp.element_size() != 4 or d_branch_of.element_size() != 4 or d_branch_of.numel() != d_logp.shape[0]:
            raise ValueError("logp must be float32 and branch_of 32-bit, one per ghost node")
        capi.check(self._lib.epik_amd_builder_add_device(self._handle, d_logp.data_ptr(), d_branch_of.data_ptr(),
                                                         int(d_logp.shape[0]), int(d_logp.shape[1])))

    def finish(self) -> SynthDB:
        keys, offsets, values, self.num_splits = _copy_out(self._lib, self._handle)
        return _as_db(self.states, self.kmer_size, self.omega, self.num_branches, self.log_thr, keys, offsets, values)

    def rank(self, filter="best", seed: int = 0):
        """(value float64 [K], order uint32 [K]) of the finished database by informativeness (epik_amd/filters.py), on the
        builder's own device arrays: after `finish`, nothing is uploaded.  `order` is what dbfile.write_db takes."""
        from . import filters
        nk, ne = ctypes.c_uint64(), ctypes.c_uint64()
        capi.check(self._lib.epik_amd_builder_finish(self._handle, ctypes.byref(nk), ctypes.byref(ne), None))
        value, order = np.zeros(nk.value, np.float64), np.zeros(nk.value, np.uint32)
        fid = filters.filter_id(filter) if isinstance(filter, str) else int(filter)
        capi.check(self._lib.epik_amd_builder_rank(self._handle, fid, int(seed) & (2 ** 64 - 1), value.ctypes.data, order.ctypes.data))
        return value, order

    def close(self) -> None:
        if self._handle:
            self._lib.epik_amd_builder_destroy(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def build_host(states: str, kmer_size: int, num_branches: int, logp, branch_of, omega: float = 1.5, log_thr=None,
               num_threads: int = 1) -> SynthDB:
    """The rule on the host (epik_amd_build_host): no device."""
    lib = capi.load()
    sigma = alphabet.alphabet_size(states)
    logp, branch_of = _chunk(logp, branch_of, sigma)
    log_thr = np.float32(default_log_thr(states, kmer_size, omega) if log_thr is None else log_thr)
    handle = ctypes.c_void_p()
    capi.check(lib.epik_amd_build_host(sigma, int(kmer_size), int(num_branches), ctypes.c_float(float(log_thr)), logp.ctypes.data,
                                       branch_of.ctypes.data, logp.shape[0], logp.shape[1], int(num_threads), ctypes.byref(handle)))
    try:
        keys, offsets, values, _ = _copy_out(lib, handle)
    finally:
        lib.epik_amd_builder_destroy(handle)
    return _as_db(states, kmer_size, omega, num_branches, log_thr, keys, offsets, values)


def _completed(s, best, at, depth, k):
    """s + the best letters of positions depth .. k - 1 of the windows at `at`, float32, left to right."""
    for j in range(depth, k):
        s = (s + best[at + j]).astype(np.float32)
    return s


def build_numpy(states: str, kmer_size: int, num_branches: int, logp, branch_of, omega: float = 1.5, log_thr=None) -> SynthDB:
    """The rule restated: per ghost node every window's k-mers level by level, float32 additions left to right from
    +0.0.  Up to UNPRUNED_CODES k-mers a window nothing is pruned; above, a frontier keeps the prefixes whose sum,
    completed left to right with the best remaining letters, reaches log_thr (the exact bound of the rule)."""
    sigma = alphabet.alphabet_size(states)
    logp, branch_of = _chunk(logp, branch_of, sigma)
    k = int(kmer_size)
    log_thr = np.float32(default_log_thr(states, k, omega) if log_thr is None else log_thr)
    G, L = logp.shape[0], logp.shape[1]
    W = L - k + 1
    prune = sigma ** k > UNPRUNED_CODES
    all_keys, all_branches, all_scores = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            node = logp[g]
            best = node.max(axis=1)
            at = np.arange(W, dtype=np.int64)               # the window of every prefix
            key = np.zeros(W, dtype=np.int64)
            s = np.zeros(W, dtype=np.float32)               # +0.0
            for j in range(k):
                s = (s[:, None] + node[at + j]).astype(np.float32).reshape(-1)
                key = (key[:, None] * sigma + np.arange(sigma, dtype=np.int64)[None, :]).reshape(-1)
                at = np.repeat(at, sigma)
                if prune and j + 1 < k:
                    alive = _completed(s, best, at, j + 1, k) >= log_thr
                    s, key, at = s[alive], key[alive], at[alive]
            keep = s >= log_thr
            all_keys.append(key[keep])
            all_scores.append(s[keep])
            all_branches.append(np.full(int(keep.sum()), int(branch_of[g]), dtype=np.int64))
    key = np.concatenate(all_keys) if all_keys else np.zeros(0, np.int64)
    branch = np.concatenate(all_branches) if all_branches else np.zeros(0, np.int64)
    score = np.concatenate(all_scores) if all_scores else np.zeros(0, np.float32)
    order = np.lexsort((-score.astype(np.float64), branch, key))   # the best score of a (key, branch) first
    key, branch, score = key[order], branch[order], score[order]
    first = np.ones(key.shape[0], dtype=bool)
    first[1:] = (key[1:] != key[:-1]) | (branch[1:] != branch[:-1])
    key, branch, score = key[first], branch[first], score[first]
    values = np.zeros(key.shape[0], dtype=PKDB_VALUE)
    values["branch"] = branch
    values["score"] = score
    keys, counts = np.unique(key, return_counts=True)
    offsets = np.zeros(keys.shape[0] + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    return _as_db(states, k, omega, num_branches, log_thr, keys.astype(np.uint32), offsets, values)
