#!/usr/bin/env python3
"""Cost of the Mantel test on the device: epik_amd_cohort_mantel_device at S = 1 000 samples over N = 999 branches, one column
side, pearson, P = 999 and P = 1, on both tiers of the permutations' vectors (LDS, and the workgroups' slices of global memory
with EPIK_AMD_MANTEL_LDS=0), beside epik_amd_cohort_kr_device (normalise + KR) of the same cohort in the same run: HIP events
around the whole call on one stream, the median of --steps after --warmup, the calls alternating.  P = 1 is the part of the call
that does not grow with P (the upload, the list, the tables, the moments) beside one chunk of permutations, so the difference of
the two is the cross-product kernel over 998 more permutations: gathered multiply-adds per second are counted from that.  The
host mirror (epik_amd_cohort_mantel_kr_host, one thread, from the device's distances) is timed once on the same input, and the
record and every stat[p] are compared byte for byte.  Spearman follows at P = 1: the cost of ranking two triangles.

    python tools/mantel_rate.py [--steps 10] [--warmup 3] [--out profiles/mantel_rate.json]

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

SWITCH = "EPIK_AMD_MANTEL_LDS"


def mantel_rates(args, num_samples, num_branches, permutations):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s, p = num_samples, permutations
    values = np.random.default_rng(44).normal(size=(1, s))
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    os.environ.pop(SWITCH, None)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = torch.zeros(2 * capi.MANTEL.itemsize, dtype=torch.uint8, device="cuda:0")
        d_stat = torch.zeros(2 * (p + 1), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()

        def mantel(perms, lds, methods=("pearson",)):
            def call():
                os.environ[SWITCH] = "1" if lds else "0"           # (read at every call)
                cohort.mantel_device(d_kr.data_ptr(), values, None, None, methods, None, perms, 1, d_out.data_ptr(), d_stat.data_ptr(),
                                     stream.cuda_stream)
            return call

        names = ("kr", "lds", "general", "lds_one", "general_one", "spearman_one")
        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream), mantel(p, True), mantel(p, False),
               mantel(1, True), mantel(1, False), mantel(1, True, ("spearman",))]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        got = {}
        for name, lds in (("lds", True), ("general", False)):
            mantel(p, lds)()
            stream.synchronize()
            got[name] = (d_out.cpu().numpy()[:capi.MANTEL.itemsize].copy(), d_stat.cpu().numpy()[:p + 1].copy())
        kr = d_kr.cpu().numpy().reshape(s, s).copy()
    os.environ.pop(SWITCH, None)
    begin = time.perf_counter()
    host = cohort_mod.mantel_kr_host(kr, cohort_mod.totals_of(mass), values, None, None, ("pearson",), None, p, 1)
    host_ms = (time.perf_counter() - begin) * 1e3
    for name, (out, stat) in got.items():
        assert out.tobytes() == host.records.tobytes() and stat.tobytes() == host.stat.tobytes(), f"{name}: device and host mirror disagree"
    ms = dict(zip(names, (round(t, 4) for t in times)))
    n = int(host.records["used"][0])
    madds = (p - 1) * n * (n - 1) // 2                              # of the permutations that P has more than the call at P = 1
    rate = {tier: round(madds / ((ms[tier] - ms[tier + "_one"]) * 1e-3)) for tier in ("lds", "general") if ms[tier] > ms[tier + "_one"]}
    return {"num_samples": s, "num_branches": num_branches, "used": n, "permutations": p, "r": float(host.records["r"][0]),
            "p": float(host.records["p"][0]), "ms": ms, "samples_ms": dict(zip(names, samples_ms)), "host_mirror_ms": round(host_ms, 1),
            "host_threads": 1, "host_over_device": {tier: round(host_ms / ms[tier], 1) for tier in ("lds", "general")},
            "results_equal_host": True, "gathered_multiply_adds": madds, "multiply_adds_per_s": rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--branches", type=int, default=999)
    ap.add_argument("--permutations", type=int, default=999)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("mantel_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "mantel_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [mantel_rates(args, args.samples, args.branches, args.permutations)]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
