#!/usr/bin/env python3
"""Cost of the device cohort.  (a) epik_amd_placer_place_device alone, place + epik_amd_profile_add_device and place +
epik_amd_cohort_add_device on device-resident reads -- the profile add on the same rows in the same run is the
yardstick --, and the adds by themselves, timed with HIP events on one stream (median of --steps after --warmup, the
variants alternating): tools/profile_rate.py's two workloads of 1 M x 150 bp on N = 999, the reads in 1, 64 and 1 024
samples, grouped, and in 1 024 samples interleaved (read i of sample i % 1024).  (b) cohort_normalise_kernel +
cohort_kr_kernel alone (epik_amd_cohort_kr_device) at S in {64, 1 024} x N in {999, 9 999} on random cells, with the
double-precision operations a second of the pairs the kernel computes (five a pair and branch: two subtractions, two
additions, one multiplication; |x| is a modifier) and of the S (S - 1) / 2 pairs asked for.

    python tools/cohort_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--out profiles/cohort_rate.json]

Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times show in the trace.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from profile_rate import timed  # noqa: E402


def add_rates(args, name, db, data, offs):
    import torch
    from epik_amd.placer import Placer
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    out = {"workload": name, "reads": n, "num_branches": int(db.num_branches)}
    layouts = [("1 sample", 1, False), ("64 samples grouped", 64, False), ("1024 samples grouped", 1024, False),
               ("1024 samples interleaved", 1024, True)]
    with Placer.from_synth(db) as pl, pl.profile() as profile:
        keep = pl.keep_at_most
        pl.choose_counts(args.read_length)
        d_seqs = torch.from_numpy(data).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
        cohorts, d_samples = [], []
        for _, num_samples, interleaved in layouts:
            ids = np.arange(n, dtype=np.int64)
            samples = (ids % num_samples if interleaved else ids * num_samples // n).astype(np.uint32)
            d_samples.append(torch.from_numpy(samples.view(np.int32)).to(dev))
            cohorts.append(pl.cohort(num_samples))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def place():
            pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), s)

        def profile_add():
            profile.add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, 0, s)

        def cohort_add(k):
            return lambda: cohorts[k].add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_samples[k].data_ptr(), n, 0, s)

        def after_place(fn):
            def both():
                place()
                fn()
            return both

        adds = [profile_add] + [cohort_add(k) for k in range(len(layouts))]
        names = ["profile"] + [layout[0] for layout in layouts]
        fns = [place] + [after_place(fn) for fn in adds] + adds
        medians, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        t_place, with_place, alone = medians[0], medians[1:1 + len(adds)], medians[1 + len(adds):]
        out["place_ms"] = round(t_place, 4)
        out["lds_path"] = bool(cohorts[0].lds_path)
        for k, label in enumerate(names):
            out[label] = {"place_and_add_ms": round(with_place[k], 4), "add_alone_ms": round(alone[k], 4),
                          "added_share_of_place": round((with_place[k] - t_place) / t_place, 4),
                          "add_alone_over_profile_add": round(alone[k] / alone[0], 3),
                          "samples_ms": {"place_and_add": samples_ms[1 + k], "add": samples_ms[1 + len(adds) + k]}}
        out["samples_ms_place"] = samples_ms[0]
        # the cells are what the profile holds, summed over the samples, however often each was added
        whole = profile.read()
        for cohort in cohorts:
            cells = cohort.read()
            assert np.array_equal(cells.mass.sum(axis=0, dtype=np.uint64), whole.mass), "cohort and profile disagree"
            cohort.close()
    return out


def kr_rates(args, num_samples, num_branches):
    import torch
    from epik_amd import synth
    from epik_amd.placer import Placer
    tree = synth.make_tree((num_branches + 1) // 2, seed=42)
    assert tree.num_nodes == num_branches
    db = synth.make_db(num_branches, kmer_size=4, seed=43)
    rng = np.random.default_rng(num_samples + num_branches)
    mass = rng.integers(0, 1 << 40, size=(num_samples, num_branches), dtype=np.uint64)
    mass[rng.random(mass.shape) < 0.5] = 0
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, tree.branch_length) as dtree, pl.cohort(num_samples) as cohort:
        cohort.add_cells(mass, None, None)
        d_out = torch.zeros(num_samples * num_samples, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()

        def kr():
            cohort.kr_device(dtree, tree.branch_length, d_out.data_ptr(), stream.cuda_stream)

        (t_kr,), samples_ms = timed(torch, stream, [kr], args.steps, args.warmup)
    side = (num_samples + 31) // 32
    computed = side * (side + 1) // 2 * 1024
    asked = num_samples * (num_samples - 1) // 2
    return {"num_samples": num_samples, "num_branches": num_branches, "normalise_and_kr_ms": round(t_kr, 4),
            "workgroups": side * (side + 1) // 2, "pairs_computed": computed, "pairs_asked": asked,
            "gflops_computed": round(5.0 * computed * num_branches / t_kr / 1e6, 1),
            "gflops_asked": round(5.0 * asked * num_branches / t_kr / 1e6, 1), "samples_ms": samples_ms[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("cohort_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance, synth
    tree = synth.make_tree(args.leaves, seed=42)
    result = {"tool": "cohort_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "add": [], "kr": []}
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    data, offs = synth.reads_hitting(db, args.reads, args.read_length, hit_rate=0.5, seed=45)
    result["add"].append(add_rates(args, "reads_hitting on bench.py's database (masses spread)", db, data, offs))
    cdb, refs, _ = synth.make_clade_db(tree.num_nodes, seed=47)
    cdata, coffs = synth.make_clade_reads(refs, args.reads, args.read_length, seed=48)
    result["add"].append(add_rates(args, "make_clade_reads on make_clade_db (masses concentrated)", cdb, cdata, coffs))
    for num_samples in (64, 1024):
        for num_branches in (999, 9999):
            result["kr"].append(kr_rates(args, num_samples, num_branches))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
