#!/usr/bin/env python3
"""Cost of the placement confidence: epik_amd_placer_place_device alone against place_device + epik_amd_confidence_device
on device-resident reads, and the confidence kernel by itself over the rows of the last placement, timed with HIP events
on one stream (median of --steps after --warmup, the variants alternating).  The workloads of tools/profile_rate.py --
1 M x 150 bp on N = 999, k = 10: bench.py's database with synth.reads_hitting reads, a synth.make_clade_db database with
make_clade_reads, one of those reads a million times; clade reads on N = 3 999 -- and the kernel alone on a ladder-shaped
tree of N = 9 999 (the deepest tree of its size: every level of an LCA query is taken) over the rows of the N = 999 clade
workload spread over it.

    python tools/assign_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--tau 0.95] [--out file.json]

Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times show in the trace.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ladder(n_nodes, seed=3):
    """A caterpillar: every inner node has one leaf and the rest of the ladder below it (post-order ids)."""
    parent = np.full(n_nodes, -1, dtype=np.int64)
    parent[0] = parent[1] = 2
    for inner in range(2, n_nodes - 2, 2):
        parent[inner] = parent[inner + 1] = inner + 2
    return parent, np.random.default_rng(seed).uniform(0.01, 0.3, size=n_nodes)


def device_rates(args, name, db, tree, data, offs, keep_rows=False):
    import torch
    from epik_amd import confidence
    from epik_amd.placer import Placer
    from profile_rate import timed
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    tau_q = confidence.tau_q(args.tau)
    out = {"workload": name, "reads": n, "num_branches": int(db.num_branches)}
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as tr:
        keep = pl.keep_at_most
        pl.choose_counts(args.read_length)
        d_seqs = torch.from_numpy(data).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
        d_conf = torch.zeros(n * 2, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def place():
            pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), s)

        def conf():
            pl.confidence_device(tr, d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, tau_q, d_conf.data_ptr(), s)

        def place_and_conf():
            place()
            conf()

        (t_place, t_both, t_conf), samples = timed(torch, stream, [place, place_and_conf, conf], args.steps, args.warmup)
        got = d_conf.cpu().numpy().view(confidence.capi.CONFIDENCE)
        n_rows = d_n.cpu().numpy().view(np.uint32)
        ok = got["clade"] < db.num_branches
        out.update(tree=tr.info(), place_ms=round(t_place, 4), place_and_confidence_ms=round(t_both, 4),
                   confidence_alone_ms=round(t_conf, 4), added_share_of_place=round((t_both - t_place) / t_place, 4),
                   confidence_bytes=int(n * (keep * 20 + 4 + 16)), confidence_gb_per_s=round(n * (keep * 20 + 20) / t_conf / 1e6, 1),
                   assigned=int(ok.sum()), mean_rows=round(float(n_rows[ok].mean()), 3) if ok.any() else 0.0,
                   clade_is_best_branch=round(float((got["clade"][ok] == d_rows.cpu().numpy().view(confidence.capi.PLACEMENT)
                                                     .reshape(n, keep)["branch"][ok, 0]).mean()), 4) if ok.any() else 0.0,
                   mean_edpl=round(float(got["edpl"][ok].mean()), 6) if ok.any() else 0.0,
                   samples_ms=dict(zip(("place", "place_and_confidence", "confidence"), samples)))
        if keep_rows:
            out["_rows"] = (d_rows.clone(), d_n.clone(), d_counts.clone())
    return out


def ladder_rate(args, rows, n_nodes):
    """The kernel alone on a ladder of n_nodes branches: the rows of a placement on a smaller tree, their branches spread
    over the ladder (b -> b * stride), so that the adjacent branches of a read lie thousands of levels apart."""
    import torch
    from epik_amd import confidence
    from profile_rate import timed
    d_rows, d_n, d_counts = rows
    n = int(d_n.shape[0])
    keep = int(d_counts.shape[0]) // n
    host = d_rows.cpu().numpy().view(confidence.capi.PLACEMENT).copy()
    small = int(host["branch"].max()) + 1
    host["branch"] = (host["branch"].astype(np.uint64) * np.uint64(n_nodes // small)).astype(np.uint32)
    spread = torch.from_numpy(host.view(np.float64)).to(d_rows.device)
    parent, lengths = ladder(n_nodes)
    d_conf = torch.zeros(n * 2, dtype=torch.float64, device=d_rows.device)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    with confidence.Tree(0, parent, lengths) as tr:
        def conf():
            tr.confidence_device(spread.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, keep, confidence.tau_q(args.tau),
                                 d_conf.data_ptr(), stream.cuda_stream)
        (t_conf,), samples = timed(torch, stream, [conf], args.steps, args.warmup)
        got = d_conf.cpu().numpy().view(confidence.capi.CONFIDENCE)
        return {"workload": f"the kernel alone on a ladder of N = {n_nodes}: the rows of the clade workload spread over it", "reads": n,
                "num_branches": n_nodes, "tree": tr.info(), "confidence_alone_ms": round(t_conf, 4),
                "assigned": int((got["clade"] < n_nodes).sum()), "samples_ms": {"confidence": samples[0]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tau", type=float, default=0.95)
    ap.add_argument("--ladder", type=int, default=9999)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("assign_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance, synth
    tree = synth.make_tree(args.leaves, seed=42)
    result = {"tool": "assign_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "tau": args.tau,
              "device": []}
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    data, offs = synth.reads_hitting(db, args.reads, args.read_length, hit_rate=0.5, seed=45)
    result["device"].append(device_rates(args, "reads_hitting on bench.py's database (masses spread)", db, tree, data, offs))
    cdb, refs, _ = synth.make_clade_db(tree.num_nodes, seed=47)
    cdata, coffs = synth.make_clade_reads(refs, args.reads, args.read_length, seed=48)
    clade = device_rates(args, "make_clade_reads on make_clade_db (masses concentrated)", cdb, tree, cdata, coffs, keep_rows=True)
    rows = clade.pop("_rows")
    result["device"].append(clade)
    one = np.tile(cdata[:args.read_length], args.reads)
    result["device"].append(device_rates(args, "one read of them, repeated", cdb, tree, one, coffs))
    big = synth.make_tree(2000, seed=42)
    bdb, brefs, _ = synth.make_clade_db(big.num_nodes, seed=47)
    bdata, boffs = synth.make_clade_reads(brefs, args.reads, args.read_length, seed=48)
    result["device"].append(device_rates(args, "make_clade_reads on make_clade_db, N = 3 999", bdb, big, bdata, boffs))
    result["device"].append(ladder_rate(args, rows, args.ladder))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
