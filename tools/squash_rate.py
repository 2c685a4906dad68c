#!/usr/bin/env python3
"""Cost of squash clustering on the device: epik_amd_cohort_squash_device -- the normalise and distance kernels, then all
S - 1 steps of three kernels each, enqueued up front -- against epik_amd_cohort_kr_device alone (the matrix the clustering
starts from) in the same run, timed with HIP events on one stream (median of --steps after --warmup, the two
alternating), at S in {64, 1 024} x N in {999, 9 999} on random cells; and against the host mirror
(epik_amd_cohort_squash_host, single-threaded, O(S^2 N)) on the same input, run once and only at S = 64, where the
records of the two are compared as well.

    python tools/squash_rate.py [--steps 10] [--warmup 3] [--out profiles/squash_rate.json]

Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times show in the trace.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from profile_rate import timed  # noqa: E402

HOST_SAMPLES = 64  # the host mirror is run at this S only


def squash_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    rng = np.random.default_rng(num_samples + num_branches)
    mass = rng.integers(0, 1 << 40, size=(num_samples, num_branches), dtype=np.uint64)
    mass[rng.random(mass.shape) < 0.5] = 0
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as dtree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(num_samples * num_samples, dtype=torch.float64, device="cuda:0")
        d_merges = torch.zeros((num_samples - 1) * 32 + 4, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def kr():
            cohort.kr_device(dtree, tree.branch_length, d_kr.data_ptr(), stream.cuda_stream)

        def squash():
            cohort.squash_device(dtree, tree.branch_length, d_merges.data_ptr(), d_merges.data_ptr() + (num_samples - 1) * 32,
                                 stream.cuda_stream)

        (t_kr, t_squash), samples_ms = timed(torch, stream, [kr, squash], args.steps, args.warmup)
        raw = d_merges.cpu().numpy()
        records = raw[:(num_samples - 1) * 32].view(capi.SQUASH_MERGE)
        count = int(raw[(num_samples - 1) * 32:].view(np.uint32)[0])
    out = {"num_samples": num_samples, "num_branches": num_branches, "merges": count, "launches": 3 + 3 * (num_samples - 1),
           "normalise_and_kr_ms": round(t_kr, 4), "squash_ms": round(t_squash, 4), "squash_over_kr": round(t_squash / t_kr, 1),
           "ms_per_step": round((t_squash - t_kr) / max(1, num_samples - 1), 5), "samples_ms": {"kr": samples_ms[0], "squash": samples_ms[1]}}
    if num_samples == HOST_SAMPLES:
        first = cohort_mod.first_of(tree.parent)
        begin = time.perf_counter()
        host = cohort_mod.squash_host(mass, first, tree.branch_length)
        out["host_mirror_ms"] = round((time.perf_counter() - begin) * 1e3, 2)
        out["host_over_device"] = round(out["host_mirror_ms"] / t_squash, 2)
        assert count == len(host) and records[:count].tobytes() == host.tobytes(), "device and host mirror disagree"
        out["records_equal_host"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("squash_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "squash_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "squash": []}
    for num_samples in (64, 1024):
        for num_branches in (999, 9999):
            result["squash"].append(squash_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
