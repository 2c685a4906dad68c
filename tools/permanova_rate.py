#!/usr/bin/env python3
"""Cost of PERMANOVA on the device: epik_amd_cohort_permanova_device (the squares, the lists, the observed labelling, the
permutations, the finish) for one column of G = 4 balanced groups at S = 1 024 samples over N = 9 999 branches, with
P = 999 and P = 9 999 permutations, beside epik_amd_cohort_kr_device (normalise + KR) of the same cohort in the same run: HIP
events around the whole call on one stream, the median of --steps after --warmup, the three alternating.  The host mirror
(epik_amd_cohort_permanova_kr_host, one thread, from the device's distances) is timed once for each P on the same input, and
the records are compared byte for byte.  Counted from the shapes: the compare-and-adds, P L (L - 1) / 2, and the bytes of
squared distances read, 8 L (L - 1) / 2 for every four permutations.

    python tools/permanova_rate.py [--steps 10] [--warmup 3] [--out profiles/permanova_rate.json]

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

PERMUTATIONS = (999, 9999)
LABELLINGS = 4  # a workgroup carries four labellings through one pass over the squared distances (permanova_place.hip: kPerms)


def permanova_rates(args, num_samples, num_branches, groups):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    labels = np.ascontiguousarray((np.random.default_rng(95).permutation(num_samples) % groups).astype(np.uint32)[:, None])
    s = num_samples
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = {p: torch.zeros(56, dtype=torch.uint8, device="cuda:0") for p in PERMUTATIONS}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()

        def permanova_of(p):
            return lambda: cohort.permanova_device(d_kr.data_ptr(), labels, p, 1, False, d_out[p].data_ptr(), 0, 0, stream.cuda_stream)

        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)] + [permanova_of(p) for p in PERMUTATIONS]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        raw = {p: d_out[p].cpu().numpy().view(capi.PERMANOVA).copy() for p in PERMUTATIONS}
        kr = d_kr.cpu().numpy().reshape(s, s).copy()
    names = ["kr"] + [f"p{p}" for p in PERMUTATIONS]
    used = int((mass.sum(axis=1) != 0).sum())
    pairs = used * (used - 1) // 2
    out = {"num_samples": s, "num_branches": num_branches, "groups": groups, "used": used,
           "ms": {k: round(t, 4) for k, t in zip(names, times)}, "over_kr": {k: round(t / times[0], 3) for k, t in zip(names[1:], times[1:])},
           "samples_ms": dict(zip(names, samples_ms)), "host_mirror_ms": {}, "host_over_device": {}, "records_equal_host": {},
           "compare_adds": {}, "compare_adds_per_s": {}, "squares_read_bytes": {}, "squares_read_bytes_per_s": {}, "p": {}}
    totals = cohort_mod.totals_of(mass)
    for p in PERMUTATIONS:
        begin = time.perf_counter()
        host = cohort_mod.permanova_kr_host(kr, totals, labels, p, 1, False, with_ssw=False)
        k = f"p{p}"
        out["host_mirror_ms"][k] = round((time.perf_counter() - begin) * 1e3, 1)
        assert raw[p].tobytes() == host.records.tobytes(), f"P = {p}: device and host mirror disagree"
        out["records_equal_host"][k] = True
        out["host_over_device"][k] = round(out["host_mirror_ms"][k] / out["ms"][k], 1)
        out["compare_adds"][k] = (p + 2) * pairs
        out["compare_adds_per_s"][k] = round(out["compare_adds"][k] / (out["ms"][k] * 1e-3))
        out["squares_read_bytes"][k] = 8 * pairs * (1 + -(-p // LABELLINGS))
        out["squares_read_bytes_per_s"][k] = round(out["squares_read_bytes"][k] / (out["ms"][k] * 1e-3))
        out["p"][k] = float(host.records["p"][0, 0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=9999)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("permanova_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "permanova_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [permanova_rates(args, args.samples, args.branches, args.groups)]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
