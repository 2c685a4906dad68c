#!/usr/bin/env python3
"""Cost of the sequential model on the device: epik_amd_cohort_model_device (the lists, the Gower matrix, the basis, the
observed sums, the permutations, the finish) for designs of R = 1, 4, 8 and 32 covariates at S = L = 1 024 samples over
N = 9 999 branches, with P = 999 and P = 9 999 permutations, beside epik_amd_cohort_permanova_device (one column of four groups)
on the same distances in the same run: HIP events around the whole call on one stream, the median of --steps after --warmup,
the calls alternating.  The host mirror (epik_amd_cohort_model_kr_host, one thread, from the device's distances) is timed once
where R * P is at most --host-work, and there the records are compared byte for byte.  Counted from the shapes: the FP64
multiply-and-adds, (P + 1) R L^2 (a multiply and an add each, never fused), and the bytes of B read, 8 L^2 for every four
permutations and every pass of eight columns (four in a design of up to four).

    python tools/model_rate.py [--steps 10] [--warmup 3] [--out profiles/model_rate.json]

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
RANKS = (1, 4, 8, 32)
PERMS, CHUNK, SMALL_COLUMNS = 4, 8, 4  # model_place.hip: kPerms, kChunk, kSmallColumns


def design_of(rank, num_samples, covariates, rng):
    """(kind, labels, values) of rank `rank`: covariates, one a term, up to 16 terms; beyond, a factor of `rank` groups (rank - 1
    columns) and one covariate."""
    if rank <= 16:
        return np.ones(rank, dtype=np.uint32), np.zeros((num_samples, rank), dtype=np.uint32), np.ascontiguousarray(covariates[:, :rank])
    labels = np.zeros((num_samples, 2), dtype=np.uint32)
    labels[:, 0] = rng.permutation(num_samples) % rank
    return np.array([0, 1], dtype=np.uint32), labels, np.ascontiguousarray(covariates[:, :2])


def model_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import capi, cohort as cohort_mod, synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    mass = cells(num_samples, num_branches)
    s = num_samples
    rng = np.random.default_rng(96)
    covariates = rng.normal(size=(s, max(RANKS)))
    groups = np.ascontiguousarray((rng.permutation(s) % 4).astype(np.uint32)[:, None])
    designs = {r: design_of(r, s, covariates, rng) for r in RANKS}
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    cases = [(r, p) for p in PERMUTATIONS for r in RANKS]
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        d_out = {c: torch.zeros((len(designs[c[0]][0]) + 1) * 48 + 40 + 64, dtype=torch.uint8, device="cuda:0") for c in cases}
        d_permanova = {p: torch.zeros(56, dtype=torch.uint8, device="cuda:0") for p in PERMUTATIONS}
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()

        def model_of(case):
            r, p = case
            base, records = d_out[case].data_ptr(), (len(designs[r][0]) + 1) * 48
            return lambda: cohort.model_device(d_kr.data_ptr(), *designs[r], p, 1, base, base + records, base + records + 40, 0,
                                               stream.cuda_stream)

        def permanova_of(p):
            return lambda: cohort.permanova_device(d_kr.data_ptr(), groups, p, 1, False, d_permanova[p].data_ptr(), 0, 0, stream.cuda_stream)

        fns = [permanova_of(p) for p in PERMUTATIONS] + [model_of(c) for c in cases]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        raw = {c: d_out[c].cpu().numpy().copy() for c in cases}
        kr = d_kr.cpu().numpy().reshape(s, s).copy()
    names = [f"permanova_p{p}" for p in PERMUTATIONS] + [f"r{r}_p{p}" for r, p in cases]
    used = int((mass.sum(axis=1) != 0).sum())
    out = {"num_samples": s, "num_branches": num_branches, "used": used, "ms": {k: round(t, 4) for k, t in zip(names, times)},
           "samples_ms": dict(zip(names, samples_ms)), "over_permanova": {}, "host_mirror_ms": {}, "host_over_device": {},
           "records_equal_host": {}, "multiply_adds": {}, "multiply_adds_per_s": {}, "b_read_bytes": {}, "b_read_bytes_per_s": {}}
    totals = cohort_mod.totals_of(mass)
    for (r, p), ms in zip(cases, times[len(PERMUTATIONS):]):
        k = f"r{r}_p{p}"
        out["over_permanova"][k] = round(ms / out["ms"][f"permanova_p{p}"], 2)
        passes = 1 if r <= SMALL_COLUMNS else -(-r // CHUNK)
        out["multiply_adds"][k] = (p + 1) * r * used * used
        out["multiply_adds_per_s"][k] = round(out["multiply_adds"][k] / (ms * 1e-3))
        out["b_read_bytes"][k] = 8 * used * used * passes * (1 + -(-p // PERMS))
        out["b_read_bytes_per_s"][k] = round(out["b_read_bytes"][k] / (ms * 1e-3))
        if r * p > args.host_work:
            continue
        begin = time.perf_counter()
        host = cohort_mod.model_kr_host(kr, totals, *designs[r], p, 1, with_stat=False)
        out["host_mirror_ms"][k] = round((time.perf_counter() - begin) * 1e3, 1)
        got = raw[(r, p)]
        want = host.records.tobytes() + host.info.tobytes() + host.aliased.tobytes()
        assert got.tobytes() == want, f"R = {r}, P = {p}: device and host mirror disagree"
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
    ap.add_argument("--host-work", type=int, default=8000, help="the host mirror runs where R * P is at most this")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("model_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance
    result = {"tool": "model_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup,
              "cases": [model_rates(args, args.samples, args.branches)]}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
