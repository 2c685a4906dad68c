#!/usr/bin/env python3
"""Cost of the device profile: epik_amd_placer_place_device alone against place_device + epik_amd_profile_add_device on
device-resident reads, timed with HIP events on one stream (median of --steps after --warmup, the two alternating), and
the add kernel by itself over the rows of the last placement -- LDS path and global path.  Two workloads of 1 M x 150 bp
on N = 999, k = 10 (BASELINE configs[1]): bench.py's database with synth.reads_hitting reads (masses spread over the
tree), a synth.make_clade_db database with make_clade_reads (masses concentrated on the reads' home clades), and one of
those reads a million times (every lane of every wave on the same cells: the contention bound); and clade reads on a
tree of N = 3 999, whose accumulators take a CU's LDS for one workgroup.

    python tools/profile_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--out file.json] [--e2e]

--e2e adds FASTA -> jplace against FASTA -> profile (--profile-only) of the driver on tools/e2e_bench.py's input.
Prints one JSON line.  Under `rocprofv3 --kernel-trace --stats` the kernels' own times show in the trace.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, stream, fns, steps, warmup):
    """Median milliseconds of each callable, the callables alternating inside every step."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    stream.synchronize()
    ms = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            fn()
            stop.record(stream)
            stop.synchronize()
            ms[k].append(start.elapsed_time(stop))
    return [statistics.median(m) for m in ms], [[round(x, 4) for x in m] for m in ms]


def device_rates(args, name, db, data, offs):
    import torch
    from epik_amd.placer import Placer
    n = len(offs) - 1
    dev = torch.device("cuda", 0)
    out = {"workload": name, "reads": n, "num_branches": int(db.num_branches)}
    for path in ("lds", "global"):
        os.environ["EPIK_AMD_PROFILE_LDS"] = "1" if path == "lds" else "0"
        with Placer.from_synth(db) as pl, pl.profile() as profile:
            keep = pl.keep_at_most
            pl.choose_counts(args.read_length)
            d_seqs = torch.from_numpy(data).to(dev)
            d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
            d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
            d_n = torch.zeros(n, dtype=torch.int32, device=dev)
            d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            stream = torch.cuda.current_stream()
            s = stream.cuda_stream

            def place():
                pl.place_device(d_seqs.data_ptr(), d_offs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), s)

            def add():
                profile.add_device(d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(), n, 0, s)

            def place_and_add():
                place()
                add()

            (t_place, t_both, t_add), samples = timed(torch, stream, [place, place_and_add, add], args.steps, args.warmup)
            got = profile.read()
            top = np.sort(got.best)[::-1]
            out[path] = {"place_ms": round(t_place, 4), "place_and_add_ms": round(t_both, 4), "add_alone_ms": round(t_add, 4),
                         "added_share_of_place": round((t_both - t_place) / t_place, 4),
                         "add_bytes": int(n * (keep * 20 + 4)), "add_gb_per_s": round(n * (keep * 20 + 4) / t_add / 1e6, 1),
                         "samples_ms": dict(zip(("place", "place_and_add", "add"), samples))}
            out["placed"], out["no_hit"] = got.totals["placed"], got.totals["no_hit"]
            out["best_share_of_top_8_branches"] = round(float(top[:8].sum()) / max(1.0, float(got.best.sum())), 4)
    os.environ.pop("EPIK_AMD_PROFILE_LDS", None)
    return out


def e2e(args):
    """FASTA -> jplace against FASTA -> profile, tools/e2e_bench.py's database and reads."""
    from epik_amd import dbfile, synth
    from e2e_bench import write_fasta
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tmp = tempfile.mkdtemp(prefix="epik_profile_")
    tree = synth.make_tree(args.leaves, seed=42)
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    db_path, fasta = os.path.join(tmp, "db.ekdb"), os.path.join(tmp, "reads.fasta")
    dbfile.write_db(db_path, db, tree.newick())
    data, _ = synth.make_reads(args.e2e_reads, 150, seed=44)
    write_fasta(fasta, data, args.e2e_reads, 150)
    out = {"reads": args.e2e_reads, "jobs": args.jobs, "batch_size": args.batch_size}
    for name, extra in (("jplace", []), ("profile_only", ["--profile-only"]), ("jplace_and_profile", ["--profile"])):
        rates = []
        for rep in range(args.e2e_repeats):
            out_dir = os.path.join(tmp, f"{name}_{rep}")
            os.makedirs(out_dir)
            run = subprocess.run([os.path.join(ROOT, "epik_amd", "bin", "epik-dna"), "-d", db_path, "-q", fasta, "-o", out_dir,
                                  "--batch-size", str(args.batch_size), "-j", str(args.jobs)] + extra, capture_output=True, text=True)
            if run.returncode != 0:
                print(run.stdout[-1500:], run.stderr[-1500:])
                raise SystemExit(run.returncode)
            ms = int(re.search(r"Placement time: .*\((\d+) ms\)", run.stdout).group(1))
            rates.append(args.e2e_reads / (ms / 1e3))
        out[name] = {"reads_per_s": round(statistics.median(rates)), "runs": [round(r) for r in rates]}
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--leaves", type=int, default=500)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--e2e-reads", type=int, default=1_000_000)
    ap.add_argument("--e2e-repeats", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=100_000)
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    if not torch.cuda.is_available():
        raise SystemExit("profile_rate.py measures on a GPU: none is visible")
    from epik_amd import provenance, synth
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    tree = synth.make_tree(args.leaves, seed=42)
    result = {"tool": "profile_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "device": []}
    db = synth.make_db(tree.num_nodes, kmer_size=10, seed=43)
    data, offs = synth.reads_hitting(db, args.reads, args.read_length, hit_rate=0.5, seed=45)
    result["device"].append(device_rates(args, "reads_hitting on bench.py's database (masses spread)", db, data, offs))
    cdb, refs, _ = synth.make_clade_db(tree.num_nodes, seed=47)
    cdata, coffs = synth.make_clade_reads(refs, args.reads, args.read_length, seed=48)
    result["device"].append(device_rates(args, "make_clade_reads on make_clade_db (masses concentrated)", cdb, cdata, coffs))
    one = np.tile(cdata[:args.read_length], args.reads)
    result["device"].append(device_rates(args, "one read of them, repeated (every lane on the same cells)", cdb, one, coffs))
    big = synth.make_tree(2000, seed=42)
    bdb, brefs, _ = synth.make_clade_db(big.num_nodes, seed=47)
    bdata, boffs = synth.make_clade_reads(brefs, args.reads, args.read_length, seed=48)
    result["device"].append(device_rates(args, "make_clade_reads on make_clade_db, N = 3 999 (a workgroup per CU)", bdb, bdata, boffs))
    if args.e2e:
        result["e2e"] = e2e(args)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
