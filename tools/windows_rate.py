#!/usr/bin/env python3
"""Cost of painting by windows: long sequences cut from the references of a clade database, W = 300, S = 75, through the
synchronous host entries, a host clock around each call (every one ends in a device synchronise).  The variants alternate
inside every round, so drift of the device shows in all of them alike:
    precut           the same windows cut on the host (not timed) and placed by Placer.place_packed: the baseline, what a
                     user does without place_windows
    windows          Placer.place_windows: count, scan and cut on the device, the placement, the rows copied out
    painted          Placer.place_and_paint_windows: the same with the paint kernel on every chunk's device rows
    painted_no_rows  ... and the rows left on the device: only records, segments, strands and offsets cross back

    python tools/windows_rate.py [--sequences 2048] [--length 10000] [--window 300] [--step 75] [--steps 7] [--warmup 2]
                                 [--out file.json]

Prints one JSON line: per variant the median, the smallest and the largest milliseconds and the windows placed per second
at the median, the cost of cut (windows - precut) and of paint (painted - windows), and whether the rows are the same
bytes.  Under `rocprofv3 --kernel-trace --stats` the kernels' own shares show in the trace.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=2048)
    ap.add_argument("--length", type=int, default=10000)
    ap.add_argument("--window", type=int, default=300)
    ap.add_argument("--step", type=int, default=75)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    from epik_amd import capi, synth, windows
    from epik_amd.placer import Placer
    if capi.device_count() < 1:
        raise SystemExit("windows_rate.py needs a HIP device: nothing is measured without one")
    tree = synth.make_tree(args.leaves, seed=42)
    N = tree.num_nodes
    # references as long as the sequences: a sequence is a reference with one letter in a hundred replaced
    db, refs, _ = synth.make_clade_db(N, kmer_size=10, n_refs=64, ref_length=args.length, seed=47)
    data, offs = synth.make_clade_reads(refs, args.sequences, args.length, seed=48)
    w, s = args.window, args.step
    wdata, woffs, wo = windows.slice_windows(data, offs, w, s)
    total = int(wo[-1])
    group = (np.arange(N) * 4 // N).astype(np.uint32)
    tau_q = windows.tau_q_of(0.8)
    with Placer.from_synth(db) as pl:
        kept = {}

        def precut():
            kept["precut"] = pl.place_packed(wdata, woffs)

        def cut_on_device():
            kept["windows"] = pl.place_windows(data, offs, w, s, "forward")

        def painted():
            kept["painted"] = pl.place_and_paint_windows(data, offs, w, s, group, tau_q, "forward")

        def painted_no_rows():
            kept["painted_no_rows"] = pl.place_and_paint_windows(data, offs, w, s, group, tau_q, "forward", rows_out=False)

        variants = (("precut", precut), ("windows", cut_on_device), ("painted", painted), ("painted_no_rows", painted_no_rows))
        times = {name: [] for name, _ in variants}
        for round_ in range(args.warmup + args.steps):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if round_ >= args.warmup:
                    times[name].append((t1 - t0) * 1e3)
        same = all(a.tobytes() == b.tobytes() for a, b in zip(kept["precut"], kept["windows"][:3]))
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(kept["windows"], kept["painted"][:5]))
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(kept["painted"][5:], kept["painted_no_rows"][5:]))
        called = float((kept["painted"][5]["call"] < capi.WINDOW_AMBIGUOUS).mean())
    med = {name: statistics.median(ms) for name, ms in times.items()}
    line = {"workload": f"clade database nucl k=10 N={N}, {args.sequences} sequences of {args.length} characters, W={w} S={s}: "
                        f"{total} windows, host buffers in and out",
            "windows": total, "steps": args.steps, "warmup": args.warmup, "median_ms": med,
            "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
            "windows_per_second": {k: total / (v * 1e-3) for k, v in med.items()},
            "cut_ms": med["windows"] - med["precut"], "paint_ms": med["painted"] - med["windows"],
            "cut_plus_paint_ms": med["painted"] - med["precut"], "same_bytes": bool(same), "windows_called": called, "all_ms": times}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
