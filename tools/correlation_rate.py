#!/usr/bin/env python3
"""Cost of the edge correlation and of the edge dispersion on the device: epik_amd_cohort_correlation_device (the normalise
kernel, the masses as a plane, the lists, the column side and the branch kernel) with M = 1 and M = 8 columns without a
missing value and with M = 8 columns of two patterns of missing values (two sets U_c, hence every branch ranked twice), and
epik_amd_cohort_dispersion_device, beside epik_amd_cohort_kr_device (normalise + KR) in the same run: HIP events around the
whole call on one stream, the median of --steps after --warmup, the variants alternating, at S in {64, 1 024} x N in
{999, 9 999} on cells drawn as reads are (most branches of a sample hold nothing, so ties dominate the ranks).  At S = 64
the host mirror (epik_amd_cohort_correlation_host / _dispersion_host) is timed once on the same input and the bytes are
compared and counted.

    python tools/correlation_rate.py [--steps 10] [--warmup 3] [--out profiles/correlation_rate.json]

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

from profile_rate import timed  # noqa: E402

HOST_SAMPLES = 64  # the host mirror is run at this S only


def cells(num_samples, num_branches):
    """mass: every sample holds 20 000 reads drawn from one of eight compositions"""
    rng = np.random.default_rng(93 + num_samples + num_branches)
    shares = rng.dirichlet(np.full(num_branches, 0.05), size=8)
    reads = np.stack([rng.multinomial(20000, shares[i % 8]) for i in range(num_samples)]).astype(np.uint64)
    return reads << np.uint64(20)


def columns(num_samples):
    """name -> meta[S][M]"""
    rng = np.random.default_rng(94 + num_samples)
    full = rng.normal(size=(num_samples, 8)) * 2.0 + 7.0
    full[:, 1::2] = np.round(full[:, 1::2])
    holes = full.copy()
    holes[rng.random(num_samples) < 0.2, 4:] = np.nan
    return {"m1": np.ascontiguousarray(full[:, :1]), "m8": full, "m8_two_patterns": holes}


def correlation_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    metas = columns(num_samples)
    s, n = num_samples, num_branches
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = {k: torch.zeros(m.shape[1] * n * 4, dtype=torch.float64, device="cuda:0") for k, m in metas.items()}
        d_used = torch.zeros(8, dtype=torch.int32, device="cuda:0")
        d_disp = torch.zeros(n * 8, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def correlation_of(k):
            return lambda: cohort.correlation_device(dtree, metas[k], d_out[k].data_ptr(), d_used.data_ptr(), stream.cuda_stream)

        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream),
               lambda: cohort.dispersion_device(dtree, d_disp.data_ptr(), stream.cuda_stream)] + [correlation_of(k) for k in metas]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        raw = {k: d_out[k].cpu().numpy() for k in metas}
        raw_disp = d_disp.cpu().numpy()
    names = ["kr", "dispersion"] + list(metas)
    out = {"num_samples": s, "num_branches": n, "empty_cells": round(float((mass == 0).mean()), 4),
           "ms": {k: round(t, 4) for k, t in zip(names, times)}, "over_kr": {k: round(t / times[0], 3) for k, t in zip(names[1:], times[1:])},
           "samples_ms": dict(zip(names, samples_ms))}
    if s == HOST_SAMPLES:
        first = cohort_mod.first_of(tree.parent)
        out["host_mirror_ms"], out["host_over_device"], out["bytes_equal_host"] = {}, {}, {}
        for k, meta in metas.items():
            begin = time.perf_counter()
            host, _ = cohort_mod.correlation_host(mass, first, meta)
            out["host_mirror_ms"][k] = round((time.perf_counter() - begin) * 1e3, 2)
            assert raw[k].tobytes() == host.tobytes(), f"correlation {k}: device and host mirror disagree"
            out["host_over_device"][k] = round(out["host_mirror_ms"][k] / out["ms"][k], 2)
            out["bytes_equal_host"][k] = len(host.tobytes())
        begin = time.perf_counter()
        host = cohort_mod.dispersion_host(mass, first)
        out["host_mirror_ms"]["dispersion"] = round((time.perf_counter() - begin) * 1e3, 2)
        assert raw_disp.tobytes() == host.tobytes(), "dispersion: device and host mirror disagree"
        out["host_over_device"]["dispersion"] = round(out["host_mirror_ms"]["dispersion"] / out["ms"]["dispersion"], 2)
        out["bytes_equal_host"]["dispersion"] = len(host.tobytes())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("correlation_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "correlation_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "cases": []}
    for num_samples in (64, 1024):
        for num_branches in (999, 9999):
            result["cases"].append(correlation_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
