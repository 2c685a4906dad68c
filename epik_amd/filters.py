"""Ranking phylo-k-mers by informativeness (include/epik_amd.h, "Ranking phylo-k-mers by informativeness").

`rank` is the device path (libepik_amd.so: epik_amd_filter_rank, host arrays in and out), `rank_device` the same on torch
tensors that already lie on the device (epik_amd_filter_rank_device), `rank_host` the host mirror in the library
(epik_amd_filter_rank_host), `rank_numpy` an independent restatement of the rule in numpy: all give the same bytes.
`ek_exp2` / `ek_log2` restate the rule's two functions operation for operation; `math_host` runs the library's.

A database is the sparse CSR form of `build.Builder.finish`: keys uint32 [K] ascending, offsets uint64 [K + 1], values
{branch, score}.  Every function returns (value float64 [K], order uint32 [K]): the order to hand to `dbfile.write_db`.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import capi
from .synth import PKDB_VALUE

#: the filters by their id in the library (EPIK_AMD_FILTER_*)
FILTERS = ("best", "mif0", "random")
CHAINS = 64

LOG2_10 = 3.321928094887362
LN2 = 0.6931471805599453
TWO_OVER_LN2 = 2.8853900817779268
SQRT_HALF = 0.7071067811865476
#: c_j, the double nearest to 1 / j!, and d_j, the double nearest to 1 / (2 j + 1): the literals of host/filter.hpp
EXP_COEFFS = (1.0, 1.0, 0.5, 0.16666666666666666, 0.041666666666666664, 0.008333333333333333, 0.001388888888888889,
              0.0001984126984126984, 2.48015873015873e-05, 2.7557319223985893e-06, 2.755731922398589e-07, 2.505210838544172e-08,
              2.08767569878681e-09, 1.6059043836821613e-10)
LOG_COEFFS = (1.0, 0.3333333333333333, 0.2, 0.14285714285714285, 0.1111111111111111, 0.09090909090909091, 0.07692307692307693,
              0.06666666666666667, 0.058823529411764705, 0.05263157894736842, 0.047619047619047616, 0.043478260869565216)


def filter_id(name) -> int:
    if name not in FILTERS:
        raise ValueError(f"unknown filter '{name}' (one of {', '.join(FILTERS)})")
    return FILTERS.index(name)


# ---- the rule in numpy ----------------------------------------------------------------------------------------------

def ek_exp2(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        live = (x >= -1022.0) & (x <= 1023.0)
        xs = np.where(live, x, 0.0)
        n = np.rint(xs)
        y = (xs - n) * LN2
        q = np.full(x.shape, EXP_COEFFS[13])
        for j in range(12, -1, -1):
            q = q * y + EXP_COEFFS[j]
        out = np.ldexp(q, n.astype(np.int32))
        return np.where(live, out, np.where(x > 1023.0, np.inf, 0.0))


def ek_log2(z) -> np.ndarray:
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(all="ignore"):
        live = (z > 0.0) & (z != np.inf)
        m, e = np.frexp(np.where(live, z, 1.0))
        low = m < SQRT_HALF
        m = np.where(low, m * 2.0, m)
        e = np.where(low, e - 1, e)
        t = (m - 1.0) / (m + 1.0)
        u = t * t
        q = np.full(z.shape, LOG_COEFFS[11])
        for j in range(10, -1, -1):
            q = q * u + LOG_COEFFS[j]
        out = e.astype(np.float64) + (t * q) * TWO_OVER_LN2
        return np.where(live, out, np.where(z == 0.0, -np.inf, np.where(z == np.inf, np.inf, np.nan)))


def _chained_sums(terms, key_of, within, K):
    """SUM of the rule: per key the 64 interleaved chains, each in ascending entry order from +0.0, then the butterfly."""
    chains = np.zeros((K, CHAINS), dtype=np.float64)
    rounds = within // CHAINS
    for r in range(int(rounds.max()) + 1 if len(rounds) else 0):
        sel = np.flatnonzero(rounds == r)           # at most one entry per (key, chain)
        chains[key_of[sel], within[sel] % CHAINS] += terms[sel]
    h = CHAINS // 2
    while h >= 1:
        chains[:, :h] = chains[:, :h] + chains[:, h:2 * h]
        h //= 2
    return chains[:, 0].copy()


def _fid(filter) -> int:
    return filter_id(filter) if isinstance(filter, str) else int(filter)


def _arrays(keys, offsets, values):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    values = np.ascontiguousarray(values, dtype=PKDB_VALUE)
    if offsets.shape != (keys.shape[0] + 1,):
        raise ValueError(f"offsets must be [{keys.shape[0] + 1}], not {offsets.shape}")
    return keys, offsets, values


def rank_numpy(num_branches: int, log_thr, keys, offsets, values, filter, seed: int = 0):
    """The rule restated.  Refuses what the library refuses (ValueError)."""
    fid = _fid(filter)
    keys, offsets, values = _arrays(keys, offsets, values)
    if fid not in range(len(FILTERS)):
        raise ValueError(f"unknown filter {fid}")
    if int(num_branches) < 1 or not np.float32(log_thr) <= 0:
        raise ValueError("num_branches must be at least 1 and log_thr at most 0")
    K, N = keys.shape[0], int(num_branches)
    if K == 0:
        return np.zeros(0, np.float64), np.zeros(0, np.uint32)
    offs = offsets.astype(np.int64)
    if (np.diff(offs) < 0).any() or (offs > offs[-1]).any():
        raise ValueError(f"offsets are not ascending at key {int(np.flatnonzero((np.diff(offs) < 0) | (offs[1:] > offs[-1]))[0])}")
    n = np.diff(offs)
    part = values[offs[0]:offs[-1]]
    score = part["score"]
    if not (score <= 0).all():
        raise ValueError(f"values[{int(offs[0] + np.flatnonzero(~(score <= 0))[0])}].score is a NaN or above 0")
    if (part["branch"] >= N).any():
        raise ValueError(f"values[{int(offs[0] + np.flatnonzero(part['branch'] >= N)[0])}].branch is not below num_branches = {N}")
    with np.errstate(all="ignore"):
        if FILTERS[fid] == "random":
            z = np.uint64(int(seed) & (2 ** 64 - 1)) + keys.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            value = (z >> np.uint64(11)).astype(np.float64)
        elif FILTERS[fid] == "best":
            value = np.full(K, np.inf)
            full = np.flatnonzero(n)
            if len(full):
                value[full] = -np.maximum.reduceat(score, offs[full] - offs[0]).astype(np.float64)
        else:
            key_of = np.repeat(np.arange(K, dtype=np.int64), n)
            within = np.arange(len(part), dtype=np.int64) - np.repeat(offs[:-1] - offs[0], n)
            x = score.astype(np.float64) * LOG2_10
            p = ek_exp2(x)
            px = np.where(p == 0.0, 0.0, p * np.where(p == 0.0, 0.0, x))
            A, B = _chained_sums(p, key_of, within, K), _chained_sums(px, key_of, within, K)
            xt = np.float64(np.float32(log_thr)) * LOG2_10
            t = ek_exp2(xt)
            R = np.where(n < N, (N - n).astype(np.float64), 0.0) * t
            C = np.where(R == 0.0, 0.0, R * np.where(R == 0.0, 0.0, xt))
            Z = A + R
            safe = np.where(Z == 0.0, 1.0, Z)
            value = np.where(Z == 0.0, np.inf, ek_log2(safe) - ((B + C) / safe))
        value = value + 0.0                       # -0.0 counts as +0.0
    bits = value.view(np.uint64)
    image = np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))
    return value, np.argsort(image, kind="stable").astype(np.uint32)


# ---- the library ----------------------------------------------------------------------------------------------------

def math_host(x):
    """(ek_exp2(x), ek_log2(x)) by the library's host code."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    e, l = np.zeros_like(x), np.zeros_like(x)
    capi.check(capi.load().epik_amd_filter_math_host(x.ctypes.data, x.size, e.ctypes.data, l.ctypes.data))
    return e, l


def rank_host(num_branches: int, log_thr, keys, offsets, values, filter, seed: int = 0, num_threads: int = 1):
    """The rule on the host (epik_amd_filter_rank_host): no device."""
    keys, offsets, values = _arrays(keys, offsets, values)
    value, order = np.zeros(keys.shape[0], np.float64), np.zeros(keys.shape[0], np.uint32)
    capi.check(capi.load().epik_amd_filter_rank_host(int(num_branches), ctypes.c_float(float(np.float32(log_thr))), keys.ctypes.data,
                                                     offsets.ctypes.data, values.ctypes.data, keys.shape[0], _fid(filter),
                                                     int(seed) & (2 ** 64 - 1), int(num_threads), value.ctypes.data, order.ctypes.data))
    return value, order


def rank(num_branches: int, log_thr, keys, offsets, values, filter, seed: int = 0, device: int = 0):
    """The rule on the device (epik_amd_filter_rank): host arrays uploaded, ranked, copied back."""
    keys, offsets, values = _arrays(keys, offsets, values)
    value, order = np.zeros(keys.shape[0], np.float64), np.zeros(keys.shape[0], np.uint32)
    capi.check(capi.load().epik_amd_filter_rank(int(device), int(num_branches), ctypes.c_float(float(np.float32(log_thr))),
                                                keys.ctypes.data, offsets.ctypes.data, values.ctypes.data, keys.shape[0], _fid(filter),
                                                int(seed) & (2 ** 64 - 1), value.ctypes.data, order.ctypes.data))
    return value, order


def rank_device(num_branches: int, log_thr, d_keys, d_offsets, d_values, filter, seed: int = 0, d_value=None, d_order=None,
                stream: int = 0, device: int = 0):
    """The same on torch tensors of the device: d_keys int32 [K] (the bits of uint32), d_offsets int64 [K + 1], d_values
    any contiguous tensor of 8 bytes an entry; d_value float64 [K] and d_order int32 [K] are written (made when None)
    and returned.  `stream` is a raw HIP stream (torch.cuda.Stream.cuda_stream); the call returns after it has drained."""
    import torch
    K = int(d_keys.numel())
    if d_offsets.numel() != K + 1 or d_keys.element_size() != 4 or d_offsets.element_size() != 8:
        raise ValueError("d_keys must be 32-bit [K] and d_offsets 64-bit [K + 1]")
    if d_value is None:
        d_value = torch.empty(K, dtype=torch.float64, device=d_keys.device)
    if d_order is None:
        d_order = torch.empty(K, dtype=torch.int32, device=d_keys.device)
    if d_value.numel() != K or d_value.element_size() != 8 or d_order.numel() != K or d_order.element_size() != 4:
        raise ValueError("d_value must be float64 [K] and d_order 32-bit [K]")
    for tensor in (d_keys, d_offsets, d_values, d_value, d_order):
        if not tensor.is_contiguous():
            raise ValueError("the tensors must be contiguous")
    capi.check(capi.load().epik_amd_filter_rank_device(int(device), int(num_branches), ctypes.c_float(float(np.float32(log_thr))),
                                                       d_keys.data_ptr(), d_offsets.data_ptr(), d_values.data_ptr(), K, _fid(filter),
                                                       int(seed) & (2 ** 64 - 1), d_value.data_ptr(), d_order.data_ptr(), int(stream)))
    return d_value, d_order


def rank_db(db, filter, seed: int = 0, host: bool = False, num_threads: int = 1, device: int = 0):
    """(value, order) of a database in the sparse form (`db.keys` set), by the host mirror or the device."""
    args = (db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, filter, seed)
    return rank_host(*args, num_threads=num_threads) if host else rank(*args, device=device)
