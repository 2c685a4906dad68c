#!/usr/bin/env python3
"""Cost of placing pairs: the 2 n mates of n pairs as single reads through epik_amd_placer_place_device against the
n pairs through epik_amd_placer_place_mates_device (mate_join_kernel, then the placement of the joined sequences),
FORWARD and BOTH, on device-resident reads, timed with HIP events on one stream.  Workload: BASELINE configs[1]
(N = 999, k = 10 -- bench.py's database; --leaves 1000 for N = 1 999) and uniform pairs of 2 x 150 bp.

    python tools/mates_rate.py [--pairs 1048576] [--leaves 500] [--steps 10] [--warmup 3] [--out file.json]

The variants alternate inside every round, so drift of the device shows in all of them alike:
    singles        the 2 n mates, count width chosen for 150 bp (the baseline: what a user does without --mates)
    singles_wide   the same with the count width of the joined sequences (301 characters)
    joined_single  the n joined sequences, built on the host, as single reads: the pairs' placement without the join
    mates_forward  place_mates_device, FORWARD
    mates_both     place_mates_device, BOTH
Prints one JSON line: per variant the median, the smallest and the largest milliseconds, and the ratios.  Under
`rocprofv3 --kernel-trace --stats` the kernels' own shares show in the trace.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    from epik_amd import capi, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree(args.leaves, seed=42)
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    n, length = args.pairs, args.read_length
    data, offs = synth.make_reads(2 * n, length, seed=44)   # read 2 i and 2 i + 1: the mates of pair i
    # the joined sequences on the host: mate 1, '-', the reverse complement of mate 2
    complement = np.arange(256, dtype=np.uint8)
    complement[list(b"ACGT")] = list(b"TGCA")
    both_mates = data.reshape(n, 2, length)
    joined = np.concatenate([both_mates[:, 0], np.full((n, 1), ord("-"), np.uint8), complement[both_mates[:, 1, ::-1]]], axis=1)
    joined_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(2 * length + 1)
    dev = torch.device("cuda", 0)
    with Placer.from_synth(db) as pl:
        keep = pl.keep_at_most
        d_seqs = torch.from_numpy(data).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_joined = torch.from_numpy(np.ascontiguousarray(joined).reshape(-1)).to(dev)
        d_joined_offs = torch.from_numpy(joined_offs.view(np.int64)).to(dev)
        d_rows = torch.zeros(2 * n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(2 * n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(2 * n * keep, dtype=torch.int32, device=dev)
        d_strand = torch.zeros(n, dtype=torch.uint8, device=dev)
        seq_bytes = int(offs[-1])
        ws = pl.mates_workspace_bytes(n, seq_bytes, "both")
        d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def singles():
            pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), 2 * n, d_rows.data_ptr(), d_n.data_ptr(),
                            d_counts.data_ptr(), s)

        def joined_single():
            pl.place_device(d_joined.data_ptr(), d_joined_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(),
                            d_counts.data_ptr(), s)

        def mates_in(strand):
            def run():
                pl.place_mates_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, seq_bytes, strand, "fr", d_ws.data_ptr(), ws,
                                      d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_strand.data_ptr(), s)
            return run

        # (name, longest sequence the count width is chosen for, the call)
        variants = (("singles", length, singles), ("singles_wide", 2 * length + 1, singles),
                    ("joined_single", 2 * length + 1, joined_single), ("mates_forward", 2 * length + 1, mates_in("forward")),
                    ("mates_both", 2 * length + 1, mates_in("both")))
        times = {name: [] for name, _, _ in variants}
        for round_ in range(args.warmup + args.steps):
            for name, longest, fn in variants:
                pl.choose_counts(longest)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                if round_ >= args.warmup:
                    times[name].append(a.elapsed_time(b))
        narrow = int((d_n[:n].cpu().numpy().view(np.uint32) == capi.ROWS_COUNTS_TOO_NARROW).sum())
        reverse_share = float(d_strand.float().mean().item())
    med = {name: statistics.median(ms) for name, ms in times.items()}
    line = {"workload": f"nucl k=10 N={tree.num_nodes}, {n} pairs of 2 x {length} bp, device-resident",
            "steps": args.steps, "warmup": args.warmup,
            "median_ms": med, "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
            "mates_forward_over_singles": med["mates_forward"] / med["singles"],
            "mates_both_over_singles": med["mates_both"] / med["singles"],
            "mates_both_over_mates_forward": med["mates_both"] / med["mates_forward"],
            "singles_wide_over_singles": med["singles_wide"] / med["singles"],
            "join_ms": med["mates_forward"] - med["joined_single"],
            "all_ms": times, "pairs_too_narrow": narrow, "pairs_reverse_won": reverse_share}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
