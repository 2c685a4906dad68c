#!/usr/bin/env python3
"""Rate of the database builder: epik_amd.build.Builder from device-resident logp (epik_amd_builder_add_device), and
the host mirror (epik_amd_build_host) on 16 threads.

Two shapes, forged clade-like posteriors (ghost nodes of a clade share a sequence up to a few substitutions; most sites
are sure of their state, some are split between two or three):

    nucl   k = 10, omega = 1.5, 2 000 ghost nodes x 1 500 sites
    amino  k = 7,  omega = 1.5, 2 000 ghost nodes x   500 sites

The device build is timed whole -- create, every add_device (--chunk ghost nodes each), finish and the copy to the host --
by a host clock around calls that end in a device synchronise; one whole build is the warm-up, the median of --steps is
reported with every sample.  The host mirror runs ONCE on a tenth of the ghost nodes (every tenth one) and its time is
multiplied by ten: the record says so ("host_scaled_from").  The split between enumeration, sort and merge comes from a
kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/build_rate.py --shape nucl --steps 1 --warmup 0 --no-host
    python tools/build_rate.py --out profiles/build_rate.json --kernel-stats nucl=DIR/.../*kernel_stats.csv

(--kernel-stats only reads the file: Name and TotalDurationNs columns, as profiles/build_kernel_stats_<shape>.csv have them.)

Prints one JSON line.
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

SHAPES = {"nucl": dict(states="nucl", k=10, sites=1500), "amino": dict(states="amino", k=7, sites=500)}
TOPS = np.array([0.99, 0.9, 0.6, 0.4])
TOP_SHARE = np.array([0.70, 0.15, 0.10, 0.05])


def forged_posteriors(states, ghosts, sites, seed=71, clade=20):
    from epik_amd import alphabet
    sigma = alphabet.alphabet_size(states)
    rng = np.random.default_rng(seed)
    base = rng.integers(0, sigma, size=((ghosts + clade - 1) // clade, sites))
    seq = base[np.arange(ghosts) // clade]
    flip = rng.random(seq.shape) < 0.03
    seq = np.where(flip, rng.integers(0, sigma, size=seq.shape), seq)
    top = TOPS[rng.choice(len(TOPS), size=seq.shape, p=TOP_SHARE)]
    # what the best state leaves goes to two other states, 70 % and 30 %; every further state has p = 0 (logp -inf)
    step = rng.integers(1, sigma - 1, size=seq.shape)
    second, third = (seq + step) % sigma, (seq + step + 1) % sigma
    rest = 1.0 - top
    post = np.zeros(seq.shape + (sigma,))
    np.put_along_axis(post, third[..., None], (rest * 0.3)[..., None], axis=2)
    np.put_along_axis(post, second[..., None], (rest * 0.7)[..., None], axis=2)
    np.put_along_axis(post, seq[..., None], top[..., None], axis=2)
    return np.round(post, 5).astype(np.float32)


def split_from_stats(path):
    """Enumeration / sort / merge shares of a rocprofv3 kernel_stats.csv."""
    groups = {"enumeration_ns": 0, "sort_ns": 0, "merge_ns": 0, "other_ns": 0}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            if "enumerate_kernel" in name:
                groups["enumeration_ns"] += ns
            elif "radix" in name.lower() or "onesweep" in name.lower() or "histogram" in name.lower() or "sort" in name.lower():
                groups["sort_ns"] += ns
            elif any(k in name for k in ("head_flag_kernel", "reduce_kernel", "merge_rank_kernel", "merge_write_kernel", "csr_kernel",
                                         "scan", "lookback")):
                groups["merge_ns"] += ns
            else:
                groups["other_ns"] += ns
    return groups


def measure(args, name):
    import torch  # (first: its HIP runtime before libepik_amd's)
    from epik_amd import build
    shape = SHAPES[name]
    branches = args.ghosts  # a ghost node a branch
    post = forged_posteriors(shape["states"], args.ghosts, shape["sites"])
    logp = build.logp_from_posteriors(post)
    branch_of = np.arange(args.ghosts, dtype=np.uint32)
    d_logp = torch.from_numpy(logp).cuda()
    d_branch = torch.from_numpy(branch_of.view(np.int32)).cuda()
    out = dict(shape=name, states=shape["states"], k=shape["k"], omega=1.5, ghost_nodes=args.ghosts, sites=shape["sites"],
               chunk=args.chunk, workspace_bytes=args.workspace)

    def one_build():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with build.Builder(shape["states"], shape["k"], branches, omega=1.5, workspace_bytes=args.workspace) as b:
            for g in range(0, args.ghosts, args.chunk):
                b.add_device(d_logp[g:g + args.chunk], d_branch[g:g + args.chunk])
            db = b.finish()
            splits = b.num_splits
        return time.perf_counter() - t0, db, splits

    for _ in range(args.warmup):
        one_build()
    samples = []
    for _ in range(args.steps):
        seconds, db, splits = one_build()
        samples.append(seconds)
    seconds = statistics.median(samples)
    out.update(device_seconds=round(seconds, 4), device_samples=[round(s, 4) for s in samples], num_keys=int(db.keys.shape[0]),
               phylo_kmers=db.num_entries, splits=splits, ghost_nodes_per_second=round(args.ghosts / seconds, 1),
               phylo_kmers_per_second=round(db.num_entries / seconds, 1))
    if not args.no_host:
        tenth = slice(0, args.ghosts, 10)
        t0 = time.perf_counter()
        host = build.build_host(shape["states"], shape["k"], branches, logp[tenth], branch_of[tenth], omega=1.5, num_threads=16)
        host_seconds = (time.perf_counter() - t0) * 10
        out.update(host_threads=16, host_scaled_from=f"one run on every tenth ghost node ({len(branch_of[tenth])}), time x 10",
                   host_seconds_scaled=round(host_seconds, 3), host_phylo_kmers_of_the_tenth=host.num_entries,
                   host_ghost_nodes_per_second=round(args.ghosts / host_seconds, 1), device_over_host=round(host_seconds / seconds, 1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--ghosts", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=250)
    ap.add_argument("--workspace", type=int, default=8 << 30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--kernel-stats", action="append", default=[], help="SHAPE=kernel_stats.csv of a rocprofv3 run of that shape")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = sorted(SHAPES) if args.shape == "all" else [args.shape]
    record = {"tool": "tools/build_rate.py", "shapes": [measure(args, name) for name in names]}
    for item in args.kernel_stats:
        name, path = item.split("=", 1)
        for shape in record["shapes"]:
            if shape["shape"] == name:
                shape["kernel_split"] = split_from_stats(path)
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
