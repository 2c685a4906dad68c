#!/usr/bin/env python3
"""Cost of the edge principal components on the device: epik_amd_cohort_epca_device -- the normalise kernel, the centring,
the Gram matrix, the Jacobi eigensolver and the back-projection -- against epik_amd_cohort_kr_device (normalise + KR) in
the same run, timed with HIP events around the whole call on one stream (median of --steps after --warmup, the two
alternating), at S in {64, 1 024} x N in {999, 9 999} with K = 5 on random cells.  At S = 64, where the eigensolver runs
in LDS, also the forced global path (EPIK_AMD_EPCA_LDS=0) and, once, the host mirror (epik_amd_cohort_epca_host,
single-threaded), whose bytes are compared with the device's.

    python tools/epca_rate.py [--steps 10] [--warmup 3] [--out profiles/epca_rate.json] [--samples 64,1024]

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

HOST_SAMPLES = 64  # the host mirror and the forced global path are run at this S only
COMPONENTS = 5


def epca_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    rng = np.random.default_rng(num_samples + num_branches)
    mass = rng.integers(0, 1 << 40, size=(num_samples, num_branches), dtype=np.uint64)
    mass[rng.random(mass.shape) < 0.5] = 0
    k = COMPONENTS
    sizes = np.cumsum([0, k * 8, num_samples * k * 8, k * num_branches * 8, 32])
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as dtree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(num_samples * num_samples, dtype=torch.float64, device="cuda:0")
        d_out = torch.zeros(int(sizes[-1]), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        base = d_out.data_ptr()

        def kr():
            cohort.kr_device(dtree, tree.branch_length, d_kr.data_ptr(), stream.cuda_stream)

        def epca():
            cohort.epca_device(dtree, k, *(base + int(at) for at in sizes[:4]), stream.cuda_stream)

        os.environ.pop("EPIK_AMD_EPCA_LDS", None)
        (t_kr, t_epca), samples_ms = timed(torch, stream, [kr, epca], args.steps, args.warmup)
        raw = d_out.cpu().numpy()
        info = raw[int(sizes[3]):].view(capi.EPCA_INFO)[0]
        used, sweeps = int(info["used"]), int(info["sweeps"])
        lds = used <= 64
        rounds = used + used % 2 - 1
        out = {"num_samples": num_samples, "num_branches": num_branches, "components": k, "used": used, "sweeps": sweeps,
               "converged": int(info["converged"]), "eigensolver": "lds" if lds else "global",
               "launches": 9 + (1 if lds else 3 * rounds * sweeps), "normalise_and_kr_ms": round(t_kr, 4),
               "epca_ms": round(t_epca, 4), "epca_over_kr": round(t_epca / t_kr, 2),
               "samples_ms": {"kr": samples_ms[0], "epca": samples_ms[1]}}
        if num_samples == HOST_SAMPLES:
            os.environ["EPIK_AMD_EPCA_LDS"] = "0"
            (_, t_global), global_ms = timed(torch, stream, [kr, epca], args.steps, args.warmup)
            os.environ.pop("EPIK_AMD_EPCA_LDS")
            out["epca_global_path_ms"] = round(t_global, 4)
            out["global_launches"] = 9 + 3 * rounds * sweeps
            out["samples_ms"]["epca_global_path"] = global_ms[1]
            assert d_out.cpu().numpy().tobytes() == raw.tobytes(), "the LDS and the global path disagree"
            first = cohort_mod.first_of(tree.parent)
            begin = time.perf_counter()
            host = cohort_mod.epca_host(mass, first, k)
            out["host_mirror_ms"] = round((time.perf_counter() - begin) * 1e3, 2)
            out["host_over_device"] = round(out["host_mirror_ms"] / t_epca, 2)
            want = host.mu.tobytes() + host.proj.tobytes() + host.edge.tobytes() + np.asarray(host.info).tobytes()
            assert raw.tobytes() == want, "device and host mirror disagree"
            out["bytes_equal_host"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", default="64,1024")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("epca_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "epca_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "epca": []}
    for num_samples in (int(x) for x in args.samples.split(",")):
        for num_branches in (999, 9999):
            result["epca"].append(epca_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
