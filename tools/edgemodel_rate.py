#!/usr/bin/env python3
"""Cost of the edge model on the device: epik_amd_cohort_edgemodel_device (the mass plane, the lists, the basis, the observed
pass, the arranged basis, the chains, the finish) for designs of R = 1, 4, 8 and 32 covariates at S = L = 1 024 samples over
N = 9 999 branches, with P = 999 and P = 9 999 permutations, and P = 1 for the fixed part of a call, beside
epik_amd_cohort_edgetest_device (one column of four groups) and epik_amd_cohort_model_device (the same design) on the same cohort
in the same run: HIP events around the whole call on one stream, the median of --steps after --warmup, the calls alternating.
The host mirror (epik_amd_cohort_edgemodel_host, one thread) is timed once where R * P is at most --host-work, and there the
records are compared byte for byte.  Counted from the shapes: the FP64 multiply-and-adds of the chains, listed * 2 * (P + 1) * R *
L with `listed` the branches that have a defined family (a multiply and an add each, never fused; a leaf's imbalance row is
staged as zeros and counted).

    python tools/edgemodel_rate.py [--steps 10] [--warmup 3] [--out profiles/edgemodel_rate.json]

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
from model_rate import design_of  # noqa: E402
from profile_rate import timed  # noqa: E402

PERMUTATIONS = (1, 999, 9999)
RANKS = (1, 4, 8, 32)
FP64_OPS_PER_S = 39.3e12  # the figure DESIGN 3.16 measures against: a multiply-add is two of them


def edgemodel_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s, n = num_samples, num_branches
    rng = np.random.default_rng(97)
    covariates = rng.normal(size=(s, max(RANKS)))
    groups = np.ascontiguousarray((rng.permutation(s) % 4).astype(np.uint32)[:, None])
    designs = {r: design_of(r, s, covariates, rng) for r in RANKS}
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    first = cohort_mod.first_of(tree.parent)
    cases = [(r, p) for p in PERMUTATIONS for r in RANKS]
    siblings = [p for p in PERMUTATIONS if p > 1]
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = {c: torch.zeros(len(designs[c[0]][0]) * n * 144 + 152 + 64, dtype=torch.uint8, device="cuda:0") for c in cases}
        d_edgetest = torch.zeros(n * 208, dtype=torch.uint8, device="cuda:0")
        d_model = torch.zeros(17 * 48 + 40 + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()

        def edgemodel_of(case):
            r, p = case
            base, records = d_out[case].data_ptr(), len(designs[r][0]) * n * 144
            return lambda: cohort.edgemodel_device(dtree, *designs[r], p, 1, base, base + records, base + records + 152, 0, 0,
                                                   stream.cuda_stream)

        def edgetest_of(p):
            return lambda: cohort.edgetest_device(dtree, groups, p, 1, d_edgetest.data_ptr(), 0, 0, stream.cuda_stream)

        def model_of(r, p):
            base = d_model.data_ptr()
            return lambda: cohort.model_device(d_kr.data_ptr(), *designs[r], p, 1, base, base + 17 * 48, base + 17 * 48 + 40, 0, stream.cuda_stream)

        fns = [edgetest_of(p) for p in siblings] + [model_of(r, p) for p in siblings for r in RANKS] + [edgemodel_of(c) for c in cases]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        raw = {c: d_out[c].cpu().numpy().copy() for c in cases}
    names = [f"edgetest_p{p}" for p in siblings] + [f"model_r{r}_p{p}" for p in siblings for r in RANKS] + [f"r{r}_p{p}" for r, p in cases]
    used = int((mass.sum(axis=1) != 0).sum())
    out = {"num_samples": s, "num_branches": n, "used": used, "ms": {k: round(t, 4) for k, t in zip(names, times)},
           "samples_ms": dict(zip(names, samples_ms)), "over_edgetest": {}, "over_model": {}, "listed": {}, "host_mirror_ms": {},
           "host_over_device": {}, "records_equal_host": {}, "multiply_adds": {}, "multiply_adds_per_s": {}, "share_of_fp64_peak": {}}
    from epik_amd import capi
    for (r, p), ms in zip(cases, times[len(names) - len(cases):]):
        k = f"r{r}_p{p}"
        terms = len(designs[r][0])
        records = raw[(r, p)][:terms * n * 144].view(capi.EDGEMODEL).reshape(terms, n)
        listed = int((~np.isnan(records["family"]["ss"])).any(axis=(0, 2)).sum())
        out["listed"][k] = listed
        out["multiply_adds"][k] = listed * 2 * (p + 1) * r * used
        out["multiply_adds_per_s"][k] = round(out["multiply_adds"][k] / (ms * 1e-3))
        out["share_of_fp64_peak"][k] = round(2 * out["multiply_adds_per_s"][k] / FP64_OPS_PER_S, 4)
        if p > 1:
            out["over_edgetest"][k] = round(ms / out["ms"][f"edgetest_p{p}"], 2)
            out["over_model"][k] = round(ms / out["ms"][f"model_r{r}_p{p}"], 2)
        if r * p > args.host_work:
            continue
        begin = time.perf_counter()
        host = cohort_mod.edgemodel_host(mass, first, *designs[r], p, 1, with_stat=False, with_max=False)
        out["host_mirror_ms"][k] = round((time.perf_counter() - begin) * 1e3, 1)
        want = host.records.tobytes() + host.info.tobytes() + host.aliased.tobytes()
        assert raw[(r, p)].tobytes() == want, f"R = {r}, P = {p}: device and host mirror disagree"
        assert int(host.info["rank"]) == r and int(host.info["used"]) == used
        out["records_equal_host"][k] = True
        out["host_over_device"][k] = round(out["host_mirror_ms"][k] / ms, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=9999)
    ap.add_argument("--host-work", type=int, default=1000, help="the host mirror runs where R * P is at most this")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("edgemodel_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "edgemodel_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [edgemodel_rates(args, args.samples, args.branches)]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
