#!/usr/bin/env python3
"""Cost of the edge test on the device: epik_amd_cohort_edgetest_device (the mass plane, the lists, per column the observed
pass, the labellings and the chains in chunks, the finish) for one column of G = 2 and of G = 4 balanced groups at S = 1 024
samples over N = 9 999 branches, with P = 999 and P = 9 999 permutations, on dense cells and on cells with nine in ten zeroed,
beside epik_amd_cohort_kr_device (normalise + KR) of the same cohort in the same run: HIP events around the whole call on one
stream, the median of --steps after --warmup, the calls alternating.  The host mirror (epik_amd_cohort_edgetest_host, one
thread) is timed once on the same input for P = 999 (and for P = 9 999 with --host-all: ten times as long), and the records are
compared byte for byte.  Counted from the records: the chained additions of the rule, one per (defined family, labelling,
position), (P + 1) L a defined family, and their rate as a share of the vector FP64 add rate of the part (78.6 TFLOP/s of
fused multiply-adds: 39.3 T additions a second).

    python tools/edgetest_rate.py [--steps 5] [--warmup 2] [--out profiles/edgetest_rate.json]

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
GROUPS = (2, 4)
FP64_ADDS_PER_S = 78.6e12 / 2


def edgetest_rates(args, kind, mass, num_branches):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    s = mass.shape[0]
    order = np.random.default_rng(95).permutation(s)
    labels = {g: np.ascontiguousarray((order % g).astype(np.uint32)[:, None]) for g in GROUPS}
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = cohort_mod.first_of(tree.parent)
    keys = [(g, p) for g in GROUPS for p in PERMUTATIONS]
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = {k: torch.zeros(num_branches * capi.EDGETEST.itemsize, dtype=torch.uint8, device="cuda:0") for k in keys}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def edgetest_of(k):
            return lambda: cohort.edgetest_device(dtree, labels[k[0]], k[1], 1, d_out[k].data_ptr(), 0, 0, stream.cuda_stream)

        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)] + [edgetest_of(k) for k in keys]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        raw = {k: d_out[k].cpu().numpy().view(capi.EDGETEST).reshape(1, num_branches).copy() for k in keys}
    names = ["kr"] + [f"g{g}_p{p}" for g, p in keys]
    used = int((mass.sum(axis=1) != 0).sum())
    out = {"cells": kind, "num_samples": s, "num_branches": num_branches, "used": used, "nonzero_cells": round(float((mass != 0).mean()), 4),
           "ms": {k: round(t, 4) for k, t in zip(names, times)}, "over_kr": {k: round(t / times[0], 3) for k, t in zip(names[1:], times[1:])},
           "samples_ms": dict(zip(names, samples_ms)), "defined_families": {}, "defined_branches": {}, "chained_adds": {},
           "chained_adds_per_s": {}, "share_of_fp64_add_rate": {}, "host_mirror_ms": {}, "host_over_device": {}, "records_equal_host": {},
           "smallest_p_adj": {}}
    for (g, p), name in zip(keys, names[1:]):
        defined = ~np.isnan(raw[(g, p)]["family"]["eta2"][0])                   # [N][4]
        out["defined_families"][name] = int(defined.sum())
        out["defined_branches"][name] = int(defined.any(axis=1).sum())
        out["chained_adds"][name] = int(defined.sum()) * (p + 1) * used
        out["chained_adds_per_s"][name] = round(out["chained_adds"][name] / (out["ms"][name] * 1e-3))
        out["share_of_fp64_add_rate"][name] = round(out["chained_adds_per_s"][name] / FP64_ADDS_PER_S, 4)
        out["smallest_p_adj"][name] = float(np.nanmin(raw[(g, p)]["family"]["p_adj"]))
        if p == PERMUTATIONS[0] or args.host_all:
            begin = time.perf_counter()
            host = cohort_mod.edgetest_host(mass, first, labels[g], p, 1, with_stat=False, with_max=False)
            out["host_mirror_ms"][name] = round((time.perf_counter() - begin) * 1e3, 1)
            assert raw[(g, p)].tobytes() == host.records.tobytes(), f"{name}: device and host mirror disagree"
            out["records_equal_host"][name] = True
            out["host_over_device"][name] = round(out["host_mirror_ms"][name] / out["ms"][name], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=9999)
    ap.add_argument("--host-all", action="store_true", help="time the host mirror for P = 9 999 as well")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("edgetest_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    dense = cells(args.samples, args.branches)
    sparse = dense.copy()
    sparse[np.random.default_rng(96).random(sparse.shape) < 0.9] = 0
    result = {"tool": "edgetest_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [edgetest_rates(args, kind, mass, args.branches) for kind, mass in (("dense", dense), ("nine in ten zeroed", sparse))]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
