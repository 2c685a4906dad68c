#!/usr/bin/env python3
"""Cost of the taxonomic assignment on the device.  epik_amd_placer_place_device alone, place + epik_amd_cohort_add_device
(the yardstick: the cohort add on the same rows in the same run), place + epik_amd_taxonomy_add_device with and without
records, and every add by itself, timed with HIP events on one stream (median of --steps after --warmup, the variants
alternating): 1 M x 150 bp reads on N = 999 with a synth_taxonomy of 311 taxa (--ranks 5), the reads in 1, 64 and
1 024 samples, grouped, and in 1 024 samples interleaved (read i of sample i % 1024).

Last, the add under a taxonomy of the root alone beside the real one: what the lca walks and the runs cost.

    python tools/taxa_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--out profiles/taxa_rate.json]

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


def add_rates(args, name, tree, db, data, offs):
    import torch
    from epik_amd import synth, taxonomy
    from epik_amd.placer import Placer
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, args.ranks, seed=46))
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    tau_q = taxonomy.mass_tau_q(0.95)
    out = {"workload": name, "reads": n, "num_branches": int(db.num_branches), "num_taxa": taxa.num_taxa, "tau_q": tau_q}
    layouts = [("1 sample", 1, False), ("64 samples grouped", 64, False), ("1024 samples grouped", 1024, False),
               ("1024 samples interleaved", 1024, True)]
    with Placer.from_synth(db) as pl:
        keep = pl.keep_at_most
        pl.choose_counts(args.read_length)
        d_seqs = torch.from_numpy(data).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
        d_records = torch.zeros(n * 4, dtype=torch.int32, device=dev)
        cohorts, objects, d_samples = [], [], []
        for _, num_samples, interleaved in layouts:
            ids = np.arange(n, dtype=np.int64)
            samples = (ids % num_samples if interleaved else ids * num_samples // n).astype(np.uint32)
            d_samples.append(torch.from_numpy(samples.view(np.int32)).to(dev))
            cohorts.append(pl.cohort(num_samples))
            objects.append(pl.taxonomy(taxa.parent, label, num_samples))
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def place():
            pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), s)

        def cohort_add(k):
            return lambda: cohorts[k].add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), d_samples[k].data_ptr(), n, 0, s)

        def taxa_add(k, records):
            return lambda: objects[k].add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, tau_q,
                                                 d_records.data_ptr() if records else 0, 0, d_samples[k].data_ptr(), s)

        def after_place(fn):
            def both():
                place()
                fn()
            return both

        adds, names = [], []
        for k, layout in enumerate(layouts):
            adds += [cohort_add(k), taxa_add(k, True), taxa_add(k, False)]
            names += [f"{layout[0]}: {what}" for what in ("cohort add", "taxa add with records", "taxa add without records")]
        fns = [place] + [after_place(fn) for fn in adds] + adds
        medians, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
        t_place, with_place, alone = medians[0], medians[1:1 + len(adds)], medians[1 + len(adds):]
        out["place_ms"] = round(t_place, 4)
        out["lds_path"] = bool(objects[0].lds_path)
        for k, label_ in enumerate(names):
            yardstick = alone[k - k % 3]  # the cohort add of the same layout
            out[label_] = {"place_and_add_ms": round(with_place[k], 4), "add_alone_ms": round(alone[k], 4),
                           "added_share_of_place": round((with_place[k] - t_place) / t_place, 4),
                           "add_alone_over_cohort_add": round(alone[k] / yardstick, 3),
                           "add_alone_over_place": round(alone[k] / t_place, 3),
                           "samples_ms": {"place_and_add": samples_ms[1 + k], "add": samples_ms[1 + len(adds) + k]}}
        out["samples_ms_place"] = samples_ms[0]
        # what the lca walks cost: the same rows under a taxonomy of the root alone (every label 0: no walk is taken, one
        # run a read) beside the real one, 1 sample, no records, alternating
        with pl.taxonomy(np.array([-1]), np.zeros(db.num_branches, np.uint32), 1) as flat, pl.taxonomy(taxa.parent, label, 1) as real:
            def control(tx):
                return lambda: tx.add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, tau_q, 0, 0, d_samples[0].data_ptr(), s)
            (t_flat, t_real), flat_samples = timed(torch, stream, [control(flat), control(real)], args.steps, args.warmup)
            out["root-only taxonomy: taxa add without records"] = {"add_alone_ms": round(t_flat, 4), "beside_ms": round(t_real, 4),
                                                                   "samples_ms": {"add": flat_samples[0], "beside": flat_samples[1]}}
        # the cells, however often each was added to: direct[] is the cohort's mass by label -- twice, an object took the
        # adds with records and the adds without
        for cohort, tx in zip(cohorts, objects):
            mass, cells = cohort.read().mass.sum(axis=0, dtype=np.uint64), tx.read()
            by_label = np.zeros(taxa.num_taxa, np.uint64)
            np.add.at(by_label, label.astype(np.int64), mass)
            assert np.array_equal(cells.direct.sum(axis=0, dtype=np.uint64), by_label * np.uint64(2)), "taxonomy and cohort disagree"
            assert int(cells.assigned.sum(dtype=np.uint64)) == int(cells.totals["placed"].sum(dtype=np.uint64))
            cohort.close()
            tx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--ranks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("taxa_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance, synth
    tree = synth.make_tree(args.leaves, seed=42)
    result = {"tool": "taxa_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "add": []}
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    data, offs = synth.reads_hitting(db, args.reads, args.read_length, hit_rate=0.5, seed=45)
    result["add"].append(add_rates(args, "reads_hitting on bench.py's database (masses spread)", tree, db, data, offs))
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
