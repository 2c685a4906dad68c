#!/usr/bin/env python3
"""Cost of the alpha diversity indices and of the rarefaction curves on the device: epik_amd_cohort_alpha_device (the
normalise kernel, the alpha kernel and its finish) and epik_amd_cohort_rarefy_device (the normalise and counts kernels, the
rarefy kernel and its finish) at depth 1 024 with step 16 and at depth 65 536 with step 1 024 (64 output depths each),
timed with HIP events around the whole call on one stream (median of --steps after --warmup, the variants alternating), at
S in {64, 1 024} x N in {999, 9 999} on cells whose samples hold more reads than the deepest depth.  The curve's cost is
reported as recurrence steps a second -- one step is one (sample, half branch, side, depth): two multiplications and one
subtraction in FP64 -- beside the device's FP64 vector peak.  Every case is compared with the host mirror
(epik_amd_cohort_alpha_host / _rarefy_host) on the same input, run once and only at S = 64, the samples shared out over
--host-threads threads (the mirror itself is single-threaded; a sample does not depend on another): the bytes are
compared and counted.

    python tools/diversity_rate.py [--steps 10] [--warmup 3] [--out profiles/diversity_rate.json]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from profile_rate import timed  # noqa: E402

HOST_SAMPLES = 64  # the host mirror is run at this S only
DEPTHS = ((16, 64), (1024, 64))  # (depth_step, num_depths): depth 1 024 and depth 65 536
# MI355X: 256 CUs x 4 SIMDs x 16 FP64 lanes a clock x 2.4 GHz = 39.3e12 FP64 vector operations a second; an FMA counts
# two, which is the 78.6 TFLOPS of the data sheet (half the 157.3 TFLOPS of FP32).  The rule fuses nothing.
FP64_VECTOR_OPS_PER_S = 256 * 4 * 16 * 2.4e9
OPS_PER_STEP = 3


def cells(num_samples, num_branches):
    """(mass, best): every sample holds between 2 and 3 times 65 536 reads"""
    rng = np.random.default_rng(91 + num_samples + num_branches)
    shares = rng.dirichlet(np.full(num_branches, 0.3), size=8)
    best = np.stack([rng.multinomial(2 * 65536 + int(rng.integers(0, 65536)), shares[i % 8]) for i in range(num_samples)]).astype(np.uint64)
    return best << np.uint64(20), best


def host_in_threads(fn, rows, threads):
    """fn(rows[a:b]) over `threads` slices of the samples, side by side; the results in order"""
    bounds = np.linspace(0, len(rows), min(threads, len(rows)) + 1).astype(int)
    with ThreadPoolExecutor(max_workers=threads) as pool:
        return np.concatenate(list(pool.map(lambda ab: fn(rows[ab[0]:ab[1]]), zip(bounds[:-1], bounds[1:]))))


def diversity_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass, best = cells(num_samples, num_branches)
    s, n = num_samples, num_branches
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, best, None)
        d_alpha = torch.zeros(s * 5, dtype=torch.float64, device="cuda:0")
        d_curve = {d: torch.zeros(s * d[1] * 2, dtype=torch.float64, device="cuda:0") for d in DEPTHS}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def alpha():
            cohort.alpha_device(dtree, bl, d_alpha.data_ptr(), stream.cuda_stream)

        def rarefy_of(d):
            return lambda: cohort.rarefy_device(dtree, bl, d[0], d[1], d_curve[d].data_ptr(), stream.cuda_stream)

        times, samples_ms = timed(torch, stream, [alpha] + [rarefy_of(d) for d in DEPTHS], args.steps, args.warmup)
        raw_alpha = d_alpha.cpu().numpy()
        raw_curve = {d: d_curve[d].cpu().numpy() for d in DEPTHS}
    out = {"num_samples": s, "num_branches": n, "alpha_ms": round(times[0], 4), "samples_ms": {"alpha": samples_ms[0]}, "rarefy": []}
    first = cohort_mod.first_of(tree.parent)
    if s == HOST_SAMPLES:
        begin = time.perf_counter()
        host = cohort_mod.alpha_host(mass, first, bl)
        out["alpha_host_mirror_ms"] = round((time.perf_counter() - begin) * 1e3, 2)
        assert raw_alpha.tobytes() == host.tobytes(), "alpha: device and host mirror disagree"
        out["alpha_bytes_equal_host"] = len(host.tobytes())
    for i, d in enumerate(DEPTHS):
        t = times[1 + i]
        steps = s * 4 * n * d[0] * d[1]
        entry = {"depth_step": d[0], "num_depths": d[1], "depth": d[0] * d[1], "rarefy_ms": round(t, 4), "recurrence_steps": steps,
                 "steps_per_s": round(steps / (t * 1e-3), 1), "fp64_ops_per_s": round(OPS_PER_STEP * steps / (t * 1e-3), 1),
                 "share_of_fp64_vector_peak": round(OPS_PER_STEP * steps / (t * 1e-3) / FP64_VECTOR_OPS_PER_S, 4), "samples_ms": samples_ms[1 + i]}
        if s == HOST_SAMPLES:
            begin = time.perf_counter()
            host = host_in_threads(lambda rows: cohort_mod.rarefy_host(rows, first, bl, d[0], d[1]), best, args.host_threads)
            entry["host_mirror_ms"] = round((time.perf_counter() - begin) * 1e3, 2)
            entry["host_threads"] = args.host_threads
            entry["host_over_device"] = round(entry["host_mirror_ms"] / t, 2)
            assert raw_curve[d].tobytes() == host.tobytes(), "rarefy: device and host mirror disagree"
            assert (host >= 0.0).all()                       # every sample has more reads than the deepest depth
            entry["bytes_equal_host"] = len(host.tobytes())
        out["rarefy"].append(entry)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("diversity_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "diversity_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "fp64_vector_ops_per_s_peak": FP64_VECTOR_OPS_PER_S, "cases": []}
    for num_samples in (64, 1024):
        for num_branches in (999, 9999):
            result["cases"].append(diversity_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
