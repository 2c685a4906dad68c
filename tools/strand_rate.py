#!/usr/bin/env python3
"""Cost of placing both strands: epik_amd_placer_place_device against epik_amd_placer_place_strands_device with
mode BOTH (two placements, the reverse-complement kernel and the strand-select kernel), on device-resident reads,
timed with HIP events on one stream after warm-up.  Workload: BASELINE configs[1] (N = 999, k = 10, 1 M x 150 bp
uniform reads -- bench.py's database and reads).

    python tools/strand_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--out file.json]

Prints one JSON line: the median milliseconds of each call and their ratio.  Under
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
    ap.add_argument("--reads", type=int, default=1 << 20)
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
    data, offs = synth.make_reads(args.reads, args.read_length, seed=44)
    n = args.reads
    dev = torch.device("cuda", 0)
    with Placer.from_synth(db) as pl:
        keep = pl.keep_at_most
        pl.choose_counts(args.read_length)
        d_seqs = torch.from_numpy(data).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
        d_strand = torch.zeros(n, dtype=torch.uint8, device=dev)
        ws = pl.strand_workspace_bytes(n, int(offs[-1]), capi.STRAND_BOTH)
        d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def forward():
            pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(),
                            d_counts.data_ptr(), s)

        def both():
            pl.place_strands_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, capi.STRAND_BOTH, d_ws.data_ptr(), ws,
                                    d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_strand.data_ptr(), s)

        times = {}
        for name, fn in (("forward", forward), ("both", both)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            times[name] = ms
        reverse_share = float(d_strand.float().mean().item())
    fwd, bth = statistics.median(times["forward"]), statistics.median(times["both"])
    line = {"workload": f"nucl k=10 N={tree.num_nodes}, {n} x {args.read_length} bp reads, device-resident",
            "steps": args.steps, "warmup": args.warmup, "forward_ms": fwd, "both_ms": bth, "both_over_forward": bth / fwd,
            "forward_ms_all": times["forward"], "both_ms_all": times["both"], "reads_reverse_won": reverse_share}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
