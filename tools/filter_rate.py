#!/usr/bin/env python3
"""Rate of the informativeness ranking: epik_amd.filters.rank_device on a device-resident CSR database, per filter, beside
a device-to-device copy of the bytes it reads and the host mirror (epik_amd_filter_rank_host) on 16 threads.

Two forged databases in the sizes of the builder's two measured shapes:

    nucl   k = 10: 4^10 keys, about 463 postings a key (486 M postings), N = 2 000 branches
    amino  k = 7:  530 M keys, about 1.32 postings a key (701 M postings), N = 2 000 branches

Lists hold ascending branches and random scores in [log_thr, 0].  The input lies on the device before the clock starts;
every call is synchronous (it returns after its stream has drained) and is timed by the host clock; one call is the warm-up,
the median of --steps is reported with every sample.  The copy moves keys + offsets + values (what the value kernel reads)
once, device to device, timed the same way in the same run.  The host mirror runs once per filter.  The split between the
value kernel and the sort comes from a kernel trace taken in a run of its own, one filter at a time:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/filter_rate.py --shape nucl --filters mif0 --steps 1 --warmup 0 --no-host
    python tools/filter_rate.py ... --kernel-stats nucl:mif0=DIR/.../*kernel_stats.csv

(--kernel-stats only reads the file: Name and TotalDurationNs columns.)  Prints one JSON line.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"nucl": dict(keys=4 ** 10, mean=463.5, log_thr=-4.26), "amino": dict(keys=530_000_000, mean=1.32, log_thr=-7.87)}
BRANCHES = 2000


def forge_on_device(name, scale):
    """(d_keys int32 [K], d_offsets int64 [K + 1], d_values int32 [E][2]) on the device, never on the host."""
    import torch
    shape = SHAPES[name]
    K = max(1, int(shape["keys"] * scale))
    gen = torch.Generator(device="cuda").manual_seed(97)
    if name == "nucl":
        lengths = torch.randint(1, 927, (K,), device="cuda", generator=gen)                     # mean 463.5
    else:
        u = torch.rand(K, device="cuda", generator=gen)
        lengths = torch.ones(K, dtype=torch.int64, device="cuda")
        for bound, n in ((0.78, 2), (0.93, 3), (0.98, 4), (0.99, 6)):                           # mean 1.33
            lengths[u >= bound] = n
        del u
    d_offsets = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(lengths, 0, out=d_offsets[1:])
    E = int(d_offsets[-1].item())
    d_values = torch.empty((E, 2), dtype=torch.int32, device="cuda")
    step = 1 << 27
    for at in range(0, E, step):                                                                # (pieces: the temporaries stay small)
        n = min(step, E - at)
        index = torch.arange(at, at + n, device="cuda")
        owner = torch.searchsorted(d_offsets[1:], index, right=True)
        d_values[at:at + n, 0] = (index - d_offsets[owner]).to(torch.int32)                     # the branch: the place in the list
        score = torch.rand(n, device="cuda", generator=gen) * shape["log_thr"]
        d_values[at:at + n, 1] = score.to(torch.float32).view(torch.int32)
        del index, owner, score
    del lengths
    d_keys = (torch.arange(K, device="cuda", dtype=torch.int64) * 2 + 1).to(torch.int32)
    torch.cuda.synchronize()
    return d_keys, d_offsets, d_values


def split_from_stats(path):
    """Value kernel / sort shares of a rocprofv3 kernel_stats.csv; `other` is this tool's forging of the database in torch
    (its searchsorted, cumsum and element-wise kernels) and the copies."""
    groups = {"value_kernel_ns": 0, "sort_ns": 0, "other_ns": 0}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            if "filter_value_kernel" in name:
                groups["value_kernel_ns"] += ns
            elif "rocprim" in name and "trampoline_kernel" in name:   # (hipCUB's radix sort; torch's own cumsum is a lookback_scan_kernel)
                groups["sort_ns"] += ns
            else:
                groups["other_ns"] += ns
    return groups


def measure(args, name):
    import torch  # (first: its HIP runtime before libepik_amd's)
    from epik_amd import filters
    log_thr = np.float32(SHAPES[name]["log_thr"])
    d_keys, d_offsets, d_values = forge_on_device(name, args.scale)
    K, E = int(d_keys.numel()), int(d_values.shape[0])
    read_bytes = 4 * K + 8 * (K + 1) + 8 * E
    out = dict(shape=name, num_keys=K, postings=E, num_branches=BRANCHES, log_thr=float(log_thr), read_bytes=read_bytes,
               written_bytes=12 * K, filters={})
    d_value = torch.empty(K, dtype=torch.float64, device="cuda")
    d_order = torch.empty(K, dtype=torch.int32, device="cuda")

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        samples = []
        for _ in range(args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            samples.append(time.perf_counter() - t0)
        return statistics.median(samples), [round(s, 5) for s in samples]

    src = torch.empty(read_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    seconds, samples = timed(lambda: dst.copy_(src))
    out.update(copy_seconds=round(seconds, 5), copy_samples=samples, copy_gb_per_second=round(2 * read_bytes / seconds / 1e9, 1))
    del src, dst
    for fname in args.filters.split(","):
        seconds, samples = timed(lambda: filters.rank_device(BRANCHES, log_thr, d_keys, d_offsets, d_values, fname, seed=1, d_value=d_value,
                                                             d_order=d_order))
        out["filters"][fname] = dict(device_seconds=round(seconds, 5), device_samples=samples,
                                     read_gb_per_second_of_the_whole_call=round(read_bytes / seconds / 1e9, 1),
                                     over_copy=round(seconds / out["copy_seconds"], 2))
    if not args.no_host:
        keys = d_keys.cpu().numpy().view(np.uint32)
        offsets = d_offsets.cpu().numpy().view(np.uint64)
        values = d_values.cpu().numpy().view(filters.PKDB_VALUE).reshape(-1)
        for fname in args.filters.split(","):
            t0 = time.perf_counter()
            value, order = filters.rank_host(BRANCHES, log_thr, keys, offsets, values, fname, seed=1, num_threads=16)
            host_seconds = time.perf_counter() - t0
            record = out["filters"][fname]
            record.update(host_threads=16, host_seconds=round(host_seconds, 3), host_over_device=round(host_seconds / record["device_seconds"], 1))
            if args.check:   # the last device call of this filter is gone by now: rank again
                filters.rank_device(BRANCHES, log_thr, d_keys, d_offsets, d_values, fname, seed=1, d_value=d_value, d_order=d_order)
                record["same_bytes"] = bool(d_value.cpu().numpy().tobytes() == value.tobytes() and
                                            d_order.cpu().numpy().tobytes() == order.tobytes())
            del value, order
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--filters", default="best,mif0,random")
    ap.add_argument("--scale", type=float, default=1.0, help="share of the shape's keys (tests of the tool itself)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--check", action="store_true", help="also compare the device's bytes with the host mirror's")
    ap.add_argument("--kernel-stats", action="append", default=[], help="SHAPE:FILTER=kernel_stats.csv of a rocprofv3 run of that pair")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = sorted(SHAPES) if args.shape == "all" else [args.shape]
    record = {"tool": "tools/filter_rate.py", "shapes": [measure(args, name) for name in names]}
    for item in args.kernel_stats:
        pair, path = item.split("=", 1)
        name, fname = pair.split(":")
        for shape in record["shapes"]:
            if shape["shape"] == name and fname in shape["filters"]:
                shape["filters"][fname]["kernel_split"] = split_from_stats(path)
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
