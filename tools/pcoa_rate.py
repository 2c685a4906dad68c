#!/usr/bin/env python3
"""Cost of the principal coordinates on the device: epik_amd_cohort_pcoa_device (the index, the centring, the Jacobi sweeps,
the order and the coordinates) at S = 1 024 samples over N = 9 999 branches, beside epik_amd_cohort_kr_device (normalise + KR)
of the same cohort in the same run: HIP events around the whole call on one stream, the median of --steps after --warmup,
the two alternating.  The host mirror (epik_amd_cohort_pcoa_kr_host, one thread, from the device's distances) is timed once
on the same input, and mu, coord and the info block are compared byte for byte.  Counted from the shapes: the launches of the
eigensolver's global path, 3 (m - 1) a sweep, and the matrix elements a round rewrites, 3 L^2 (A twice, V once).  S = 512 and
S = 256 follow, the same launches a round over a quarter and a sixteenth of the elements: what the time of a launch does there
says whether the launches or the arithmetic cost the time.  The last case, S = 64, is the eigensolver's one-launch LDS path.
Then PERMDISP over the same distances, epik_amd_cohort_permdisp_device at S = 1 024 with one column of four balanced groups,
P = 999 and 9 999, timed the same way beside normalise + KR, its host mirror once, every output compared byte for byte; and
P = 1, which is the part of the call that does not grow with P: the upload, the lists, the distances to the centroids (a
workgroup a column) and the observed sums, beside one labelling.

    python tools/pcoa_rate.py [--steps 10] [--warmup 3] [--out profiles/pcoa_rate.json]

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

LDS_SIDE = 64  # the largest matrix the eigensolver keeps in LDS (jacobi_device.hpp: kJacobiLdsSide)


def pcoa_rates(args, num_samples, num_branches, components):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s, k = num_samples, components
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_mu = torch.zeros(s, dtype=torch.float64, device="cuda:0")
        d_coord = torch.zeros(s * k, dtype=torch.float64, device="cuda:0")
        d_info = torch.zeros(capi.PCOA_INFO.itemsize, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream),
               lambda: cohort.pcoa_device(d_kr.data_ptr(), k, d_mu.data_ptr(), d_coord.data_ptr(), d_info.data_ptr(), stream.cuda_stream)]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        mu, coord = d_mu.cpu().numpy().copy(), d_coord.cpu().numpy().reshape(s, k).copy()
        info = d_info.cpu().numpy().view(capi.PCOA_INFO)[0].copy()
        kr = d_kr.cpu().numpy().reshape(s, s).copy()
    begin = time.perf_counter()
    host = cohort_mod.pcoa_kr_host(kr, cohort_mod.totals_of(mass), k)
    host_ms = (time.perf_counter() - begin) * 1e3
    assert mu.tobytes() == host.mu.tobytes() and coord.tobytes() == host.coord.tobytes() and \
        info.tobytes() == np.asarray(host.info).tobytes(), f"S = {s}: device and host mirror disagree"
    used, sweeps = int(info["used"]), int(info["sweeps"])
    m = used + used % 2
    lds = used <= LDS_SIDE
    launches = 1 if lds else 3 * (m - 1) * sweeps
    rewritten = 3 * used * used * (m - 1) * sweeps
    pcoa_ms = times[1]
    return {"num_samples": s, "num_branches": num_branches, "components": k, "used": used, "eigensolver_path": "lds" if lds else "global",
            "sweeps": sweeps, "converged": int(info["converged"]), "negative": host.negative,
            "ms": {"kr": round(times[0], 4), "pcoa": round(pcoa_ms, 4)}, "over_kr": round(pcoa_ms / times[0], 3),
            "samples_ms": dict(zip(("kr", "pcoa"), samples_ms)), "host_mirror_ms": round(host_ms, 1),
            "host_over_device": round(host_ms / pcoa_ms, 1), "results_equal_host": True,
            "eigensolver_launches": launches, "us_per_launch": round(pcoa_ms * 1e3 / launches, 3),
            "elements_rewritten": rewritten, "elements_rewritten_per_s": round(rewritten / (pcoa_ms * 1e-3))}


def permdisp_rates(args, num_samples, num_branches, permutations):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s, p = num_samples, permutations
    labels = (np.arange(s, dtype=np.uint32) % 4)[:, None].copy()              # one column, four balanced groups
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = torch.zeros(capi.PERMDISP.itemsize, dtype=torch.uint8, device="cuda:0")
        d_stat = torch.zeros(p + 1, dtype=torch.float64, device="cuda:0")
        d_mean = torch.zeros(32, dtype=torch.float64, device="cuda:0")
        d_z = torch.zeros(s, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        fns = [lambda: cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream),
               lambda: cohort.permdisp_device(d_kr.data_ptr(), labels, p, 1, False, d_out.data_ptr(), d_mean.data_ptr(), d_z.data_ptr(),
                                              d_stat.data_ptr(), stream.cuda_stream)]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        got = [x.cpu().numpy().copy() for x in (d_out, d_stat, d_mean, d_z)]
        kr = d_kr.cpu().numpy().reshape(s, s).copy()
    begin = time.perf_counter()
    host = cohort_mod.permdisp_kr_host(kr, cohort_mod.totals_of(mass), labels, p, 1, False)
    host_ms = (time.perf_counter() - begin) * 1e3
    want = (host.records, host.stat, host.group_mean, host.z)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), f"P = {p}: device and host mirror disagree"
    record = host.records[0, 0]
    return {"num_samples": s, "num_branches": num_branches, "groups": int(record["groups"]), "permutations": p,
            "clipped": int(record["clipped"]), "eta2": float(record["eta2"]), "p": float(record["p"]),
            "ms": {"kr": round(times[0], 4), "permdisp": round(times[1], 4)}, "over_kr": round(times[1] / times[0], 3),
            "samples_ms": dict(zip(("kr", "permdisp"), samples_ms)), "host_mirror_ms": round(host_ms, 1),
            "host_over_device": round(host_ms / times[1], 1), "results_equal_host": True,
            "labellings_per_s": round(p / (times[1] * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1024, 512, 256, LDS_SIDE])
    ap.add_argument("--branches", type=int, default=9999)
    ap.add_argument("--components", type=int, default=5)
    ap.add_argument("--permdisp-samples", type=int, default=1024)
    ap.add_argument("--permdisp-permutations", type=int, nargs="*", default=[1, 999, 9999])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("pcoa_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "pcoa_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [pcoa_rates(args, s, args.branches, args.components) for s in args.samples],
              "permdisp": [permdisp_rates(args, args.permdisp_samples, args.branches, p) for p in args.permdisp_permutations]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
