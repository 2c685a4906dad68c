#!/usr/bin/env python3
"""Rate of the ancestral reconstruction: epik_amd.ancestral.Ancestral, posteriors left on the device
(epik_amd_ancestral_posteriors_device) and copied to the host (epik_amd_ancestral_posteriors), and the host mirror
(epik_amd_ancestral_host) on 16 threads.

Two shapes, a random tree and an alignment evolved along it, both ghost nodes of every branch:

    nucl   N = 9 999 (5 000 leaves), 1 500 sites, GTR+G4 (four categories)
    amino  N = 1 999 (1 000 leaves),   500 sites, POISSON+G4

The device call is timed whole by a host clock (the calls end in a device synchronise); one call is the warm-up, the
median of --steps is reported with every sample.  The bytes the rule has to move -- per node and site the partials of
two children read and one written, masks for leaves, the ghost kernel's two reads and its float32 rows -- are counted
from the tree, and set against the rate of a device-to-device copy measured in the same run.  The kernels' own time comes
from a kernel trace taken in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ancestral_rate.py --shape nucl --steps 1 --warmup 0 --no-host
    python tools/ancestral_rate.py --out profiles/ancestral_rate.json --kernel-stats nucl=DIR/.../*kernel_stats.csv

(--kernel-stats only reads the file: Name, Calls and TotalDurationNs columns.)

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

SHAPES = {"nucl": dict(states="nucl", leaves=5000, sites=1500, model="GTR{1.2/3.1/0.8/1.1/3.4/1.0}+FU{0.3/0.2/0.2/0.3}+G4{0.8}"),
          "amino": dict(states="amino", leaves=1000, sites=500, model="POISSON+G4{0.8}")}


def make_input(shape, seed=81):
    from epik_amd import alphabet, ancestral, newick, synth
    rng = np.random.default_rng(seed)
    tree = synth.make_tree(shape["leaves"], seed=seed)
    sigma = alphabet.alphabet_size(shape["states"])
    seqs = np.zeros((tree.num_nodes, shape["sites"]), dtype=np.int64)
    seqs[tree.num_nodes - 1] = rng.integers(0, sigma, size=shape["sites"])
    for v in range(tree.num_nodes - 2, -1, -1):
        redraw = rng.random(shape["sites"]) < min(0.6, 3.0 * tree.branch_length[v])
        seqs[v] = np.where(redraw, rng.integers(0, sigma, size=shape["sites"]), seqs[tree.parent[v]])
    ref = newick.parse(tree.newick())
    leaves = ref.leaves()
    masks = (np.uint32(1) << seqs[leaves].astype(np.uint32)).astype(np.uint32)
    masks[rng.random(masks.shape) < 0.03] = 0  # gaps
    model = ancestral.Model.parse(shape["model"], shape["states"]).resolve(None, masks)
    weights, p_full, p_half, p_pend = model.tables(ref)
    return ref, (ancestral.tree_parent(ref), sigma, weights, model.freqs, p_full, p_half, p_pend), masks


def bytes_of_the_rule(ref, sigma, categories, sites):
    """What the three kernels read and write of partials, masks and posteriors (the matrices are small and stay in cache)."""
    vec = categories * sigma * 8
    n = ref.num_nodes
    src = [4 if ref.is_leaf(u) else vec for u in range(n)]
    down = sum(src[c] for v in range(n) for c in ref.children[v]) + sum(vec for v in range(n) if not ref.is_leaf(v))
    up = 0
    for v in range(n - 1):
        p = ref.parent[v]
        sibling = [c for c in ref.children[p] if c != v][0]
        up += src[sibling] + (vec if p != n - 1 else 0) + vec
    ghost = sum(src[b] + vec + 2 * sigma * 4 for b in range(n - 1))
    return dict(down_bytes=down * sites, up_bytes=up * sites, ghost_bytes=ghost * sites)


def kernels_from_stats(path):
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            for key in ("down_kernel", "up_kernel", "ghost_kernel"):
                if key in name:
                    out[key + "_ns"] = out.get(key + "_ns", 0) + ns
                    out[key + "_calls"] = out.get(key + "_calls", 0) + int(float(row.get("Calls") or 0))
    return out


def copy_rate(torch, nbytes=1 << 30):
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    samples = []
    for _ in range(5):
        t0 = time.perf_counter()
        b.copy_(a)
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return 2 * nbytes / statistics.median(samples)


def measure(args, name):
    import torch  # (first: its HIP runtime before libepik_amd's)
    from epik_amd import ancestral
    shape = SHAPES[name]
    ref, inputs, masks = make_input(shape)
    sigma, categories = inputs[1], inputs[2].shape[0]
    ghosts = 2 * (ref.num_nodes - 1)
    out = dict(shape=name, states=shape["states"], model=shape["model"], num_nodes=ref.num_nodes, sites=shape["sites"],
               categories=categories, ghost_nodes=ghosts, workspace_bytes=args.workspace)
    moved = bytes_of_the_rule(ref, sigma, categories, shape["sites"])
    out.update(moved, rule_bytes=sum(moved.values()))
    t0 = time.perf_counter()
    with ancestral.Ancestral(*inputs, workspace_bytes=args.workspace) as a:
        out["create_seconds"] = round(time.perf_counter() - t0, 4)

        def timed(call):
            for _ in range(args.warmup):
                call()
            samples = []
            for _ in range(args.steps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                result = call()
                samples.append(time.perf_counter() - t)
                del result
            return statistics.median(samples), [round(s, 4) for s in samples]

        seconds, samples = timed(lambda: a.posteriors_device(masks, "both"))
        out.update(device_seconds=round(seconds, 4), device_samples=samples, ghost_nodes_per_second=round(ghosts / seconds, 1),
                   dead_rows=a.dead_sites)
        if not args.no_host:
            to_host, samples = timed(lambda: a.posteriors(masks, "both"))
            out.update(device_to_host_seconds=round(to_host, 4), device_to_host_samples=samples)
    rate = copy_rate(torch)
    out.update(copy_bytes_per_second=round(rate, 0), rule_bytes_over_call=round(out["rule_bytes"] / seconds, 0),
               call_share_of_copy_rate=round(out["rule_bytes"] / seconds / rate, 3))
    if not args.no_host:
        t0 = time.perf_counter()
        _, _, dead = ancestral.posteriors_host(*inputs, masks, "both", num_threads=16)
        host_seconds = time.perf_counter() - t0
        out.update(host_threads=16, host_seconds=round(host_seconds, 3), host_ghost_nodes_per_second=round(ghosts / host_seconds, 1),
                   host_over_device=round(host_seconds / seconds, 1), host_over_device_to_host=round(host_seconds / to_host, 1),
                   host_dead_rows=dead)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=sorted(SHAPES) + ["all"], default="all")
    ap.add_argument("--workspace", type=int, default=8 << 30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--kernel-stats", action="append", default=[], help="SHAPE=kernel_stats.csv of a rocprofv3 run of that shape")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = sorted(SHAPES) if args.shape == "all" else [args.shape]
    record = {"tool": "tools/ancestral_rate.py", "shapes": [measure(args, name) for name in names]}
    for item in args.kernel_stats:
        name, path = item.split("=", 1)
        for shape in record["shapes"]:
            if shape["shape"] == name:
                kernels = kernels_from_stats(path)
                total = sum(v for k, v in kernels.items() if k.endswith("_ns"))
                shape["kernel_trace"] = dict(kernels, kernels_seconds=round(total * 1e-9, 5),
                                             rule_bytes_over_kernels=round(shape["rule_bytes"] / (total * 1e-9), 0) if total else None)
                if total:
                    shape["kernel_trace"]["kernels_share_of_copy_rate"] = round(shape["rule_bytes"] / (total * 1e-9) / shape["copy_bytes_per_second"], 3)
    line = json.dumps(record)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
