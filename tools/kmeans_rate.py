#!/usr/bin/env python3
"""Cost of phylogenetic k-means on the device: epik_amd_cohort_kmeans_device -- the normalise kernel, the seeding (K
passes of two kernels, enqueued up front), then three kernels, one 4-byte readback and an update per iteration -- for
K in {4, 16} and max_iterations = 100, against epik_amd_cohort_kr_device (normalise + the KR matrix) and against
epik_amd_cohort_squash_device in the same run, timed with HIP events around the whole call on one stream (median of
--steps after --warmup, the variants alternating), at S in {64, 1 024} x N in {999, 9 999} on planted cells (8 groups:
sample i drawn around centre i % 8); and against the host mirror (epik_amd_cohort_kmeans_host, single-threaded) on the
same input, run once and only at S = 64.  The bytes of the device's four outputs are compared with the host mirror's at
S = 64 and counted.

    python tools/kmeans_rate.py [--steps 10] [--warmup 3] [--out profiles/kmeans_rate.json]

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
GROUPS = 8
CLUSTERS = (4, 16)
MAX_ITERATIONS = 100


def planted(num_samples, num_branches):
    rng = np.random.default_rng(77 + num_samples + num_branches)
    centres = rng.dirichlet(np.full(num_branches, 0.05), size=GROUPS)
    return np.stack([rng.multinomial(20_000, centres[i % GROUPS]) for i in range(num_samples)]).astype(np.uint64) << np.uint64(20)


def kmeans_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = planted(num_samples, num_branches)
    s, n = num_samples, num_branches
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_merges = torch.zeros((s - 1) * 32 + 4, dtype=torch.uint8, device="cuda:0")
        sizes = {k: [s * 16, k * 24, k * n * 8, 16] for k in CLUSTERS}
        d_out = {k: torch.zeros(sum(sizes[k]), dtype=torch.uint8, device="cuda:0") for k in CLUSTERS}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def kr():
            cohort.kr_device(dtree, tree.branch_length, d_kr.data_ptr(), stream.cuda_stream)

        def squash():
            cohort.squash_device(dtree, tree.branch_length, d_merges.data_ptr(), d_merges.data_ptr() + (s - 1) * 32, stream.cuda_stream)

        def kmeans_of(k):
            at = np.concatenate([[0], np.cumsum(sizes[k])])
            base = d_out[k].data_ptr()

            def run():
                cohort.kmeans_device(dtree, tree.branch_length, k, MAX_ITERATIONS, *(base + int(a) for a in at[:4]), stream.cuda_stream)
            return run

        times, samples_ms = timed(torch, stream, [kr, squash] + [kmeans_of(k) for k in CLUSTERS], args.steps, args.warmup)
        raw = {k: d_out[k].cpu().numpy() for k in CLUSTERS}
    t_kr, t_squash = times[0], times[1]
    out = {"num_samples": s, "num_branches": n, "groups": GROUPS, "normalise_and_kr_ms": round(t_kr, 4), "squash_ms": round(t_squash, 4),
           "kmeans": [], "samples_ms": {"kr": samples_ms[0], "squash": samples_ms[1]}}
    for i, k in enumerate(CLUSTERS):
        t = times[2 + i]
        info = raw[k][-16:].view(capi.KMEANS_INFO)[0]
        iterations = int(info["iterations"])
        entry = {"num_clusters": k, "kmeans_ms": round(t, 4), "iterations": iterations, "converged": int(info["converged"]),
                 "ms_per_iteration": round(t / max(1, iterations), 5), "kmeans_over_kr": round(t / t_kr, 2),
                 "kmeans_over_squash": round(t / t_squash, 4), "launches": 2 + 2 * k + 4 * iterations, "samples_ms": samples_ms[2 + i]}
        if s == HOST_SAMPLES:
            first = cohort_mod.first_of(tree.parent)
            begin = time.perf_counter()
            host = cohort_mod.kmeans_host(mass, first, tree.branch_length, k, MAX_ITERATIONS)
            entry["host_mirror_ms"] = round((time.perf_counter() - begin) * 1e3, 2)
            entry["host_over_device"] = round(entry["host_mirror_ms"] / t, 2)
            want = host.samples.tobytes() + host.clusters.tobytes() + host.centroids.tobytes() + np.asarray(host.info).tobytes()
            assert raw[k].tobytes() == want, "device and host mirror disagree"
            entry["bytes_equal_host"] = len(want)
        out["kmeans"].append(entry)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("kmeans_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "kmeans_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "max_iterations": MAX_ITERATIONS, "cases": []}
    for num_samples in (64, 1024):
        for num_branches in (999, 9999):
            result["cases"].append(kmeans_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
