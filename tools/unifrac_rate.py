#!/usr/bin/env python3
"""Cost of the UniFrac distances on the device: epik_amd_cohort_unifrac_device (normalise + cohort_unifrac_kernel) for each of
the three metrics beside epik_amd_cohort_kr_device (normalise + cohort_kr_kernel, the yardstick) of the same cohort in the
same run, at S in {64, 1 024} samples x N in {999, 9 999} branches: HIP events around the whole call on one stream, the
median of --steps after --warmup, the four alternating.  Every device matrix is compared byte for byte with the host mirror
(epik_amd_cohort_unifrac_host, one thread): the whole matrix up to --host-pairs pair-branches, beyond that the block of the
first 128 samples, which the rule makes the matrix of those samples alone.  The mirror is timed where the whole matrix is
compared.  Counted from the shapes: S (S - 1) / 2 * N pair-branches a call, so the pair-branches a second of each kernel.

    python tools/unifrac_rate.py [--steps 10] [--warmup 3] [--out profiles/unifrac_rate.json]

Prints one JSON line.
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

from correlation_rate import cells  # noqa: E402
from profile_rate import timed  # noqa: E402

METRICS = ("unweighted", "weighted", "generalized")
BLOCK = 128  # the samples of the block compared where the whole matrix would take the mirror too long


def unifrac_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s = num_samples
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = cohort_mod.first_of(tree.parent)
    names = ("kr",) + METRICS
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_out = {name: torch.zeros(s * s, dtype=torch.float64, device="cuda:0") for name in names}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        fns = [lambda: cohort.kr_device(dtree, bl, d_out["kr"].data_ptr(), stream.cuda_stream)]
        fns += [lambda name=name: cohort.unifrac_device(dtree, bl, name, d_out[name].data_ptr(), stream.cuda_stream) for name in METRICS]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        got = {name: d_out[name].cpu().numpy().reshape(s, s).copy() for name in names}
    pair_branches = s * (s - 1) // 2 * num_branches
    whole = pair_branches <= args.host_pairs
    rows = s if whole else min(s, BLOCK)
    host_ms = {}
    for name in names:
        begin = time.perf_counter()
        want = cohort_mod.kr_host(mass[:rows], first, bl) if name == "kr" else cohort_mod.unifrac_host(mass[:rows], first, bl, name)
        if whole:
            host_ms[name] = round((time.perf_counter() - begin) * 1e3, 1)
        assert np.ascontiguousarray(got[name][:rows, :rows]).tobytes() == want.tobytes(), f"S = {s}, N = {num_branches}, {name}: device and host mirror disagree"
    ms = dict(zip(names, (round(t, 4) for t in times)))
    out = {"num_samples": s, "num_branches": num_branches, "pair_branches": pair_branches, "ms": ms,
           "over_kr": {name: round(ms[name] / ms["kr"], 3) for name in METRICS},
           "pair_branches_per_s": {name: round(pair_branches / (ms[name] * 1e-3)) for name in names},
           "samples_ms": dict(zip(names, samples_ms)), "compared_with_host": "whole matrix" if whole else f"first {rows} samples",
           "results_equal_host": True}
    if whole:
        out["host_mirror_ms"] = host_ms
        out["host_over_device"] = {name: round(host_ms[name] / ms[name], 1) for name in names}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--branches", type=int, nargs="+", default=[999, 9999])
    ap.add_argument("--host-pairs", type=int, default=600_000_000, help="the most pair-branches the host mirror computes whole")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("unifrac_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "unifrac_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [unifrac_rates(args, s, n) for s in args.samples for n in args.branches]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
