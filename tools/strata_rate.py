#!/usr/bin/env python3
"""Cost of the strata rule on the device, and proof that it costs the calls without strata nothing: the four permutation tests
(epik_amd_cohort_permanova_device, _permdisp_device, _edgetest_device, _model_device; one column of G = 4 balanced groups) at
S = 1 024 samples over N = 9 999 branches with P = 999 and P = 9 999 permutations, from this tree's library and from a library
built from the parent commit, the two alternating in one run:

  1. every call without strata from both libraries: the parent's is the yardstick, and the difference should lie within the
     spread between the rounds of one library (a larger one means that the kStrata split leaked into the old instantiation);
  2. every call with strata (512 pairs; 8 blocks of 128) from this tree's library over the parent's call without: a ratio,
     no target.

HIP events around the whole call on one stream, the median of --steps after --warmup, the calls alternating inside a step
(tools/permanova_rate.py's method).  A library is loaded once a process (EPIK_AMD_LIB), so every round starts two fresh child
processes, one after the other, this tree's and the parent's.  PATH is a libepik_amd.so built from the parent commit:

    python tools/strata_rate.py --parent-lib PATH --out profiles/strata_rate.json

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PERMUTATIONS = (999, 9999)
ANALYSES = ("permanova", "permdisp", "edgetest", "model")


def measure(args):
    """One library (the process's), every call: {"has_strata", "ms": {call: median}, "samples_ms"}."""
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    from correlation_rate import cells
    from profile_rate import timed
    from epik_amd import capi, synth
    from epik_amd.placer import Placer
    lib = capi.load()
    has_strata = hasattr(lib, "epik_amd_cohort_permanova_strata_device")
    s, n = args.samples, args.branches
    tree = synth.make_tree((n + 1) // 2, seed=42)
    db = synth.make_db(n, kmer_size=4, seed=43)
    mass = cells(s, n)
    labels = np.ascontiguousarray((np.random.default_rng(95).permutation(s) % 4).astype(np.uint32)[:, None])
    kind, values = np.zeros(1, np.uint32), np.zeros((s, 1))
    layouts = {"none": None}
    if has_strata:
        layouts.update(pairs=(np.arange(s) // 2).astype(np.uint32), blocks=(np.arange(s) // 128).astype(np.uint32))
    bl = np.asarray(tree.branch_length, dtype=np.float64)
    with Placer.from_synth(db) as pl, pl.tree(tree.parent, bl) as dtree, pl.cohort(s) as cohort:
        cohort.add_cells(mass, None, None)
        d_kr = torch.zeros(s * s, dtype=torch.float64, device="cuda:0")
        buf = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        d_out, d_mean, d_z, d_info, d_aliased = buf(max(n * 208, 96)), buf(32 * 8), buf(s * 8), buf(40), buf(64)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        cohort.kr_device(dtree, bl, d_kr.data_ptr(), stream.cuda_stream)
        stream.synchronize()

        def call(analysis, p, strata):
            more = {} if strata is None else {"strata": strata}
            if analysis == "permanova":
                return lambda: cohort.permanova_device(d_kr.data_ptr(), labels, p, 1, False, d_out.data_ptr(), 0, 0, stream.cuda_stream, **more)
            if analysis == "permdisp":
                return lambda: cohort.permdisp_device(d_kr.data_ptr(), labels, p, 1, False, d_out.data_ptr(), d_mean.data_ptr(), d_z.data_ptr(),
                                                      0, stream.cuda_stream, **more)
            if analysis == "edgetest":
                return lambda: cohort.edgetest_device(dtree, labels, p, 1, d_out.data_ptr(), 0, 0, stream.cuda_stream, **more)
            return lambda: cohort.model_device(d_kr.data_ptr(), kind, labels, values, p, 1, d_out.data_ptr(), d_info.data_ptr(),
                                               d_aliased.data_ptr(), 0, stream.cuda_stream, **more)

        names = [f"{a}_p{p}_{layout}" for a in ANALYSES for p in PERMUTATIONS for layout in layouts]
        fns = [call(a, p, layouts[layout]) for a in ANALYSES for p in PERMUTATIONS for layout in layouts]
        times, samples_ms = timed(torch, stream, fns, args.steps, args.warmup)
    return {"has_strata": has_strata, "ms": {k: round(t, 4) for k, t in zip(names, times)}, "samples_ms": dict(zip(names, samples_ms))}


def child(args, lib_path):
    env = dict(os.environ)
    if lib_path:
        env["EPIK_AMD_LIB"] = lib_path
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup), "--samples",
            str(args.samples), "--branches", str(args.branches)]
    run = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise SystemExit(f"the child with {lib_path or 'this library'} failed:\n{run.stdout[-2000:]}{run.stderr[-2000:]}")
    return json.loads(run.stdout.strip().splitlines()[-1])


def spread(values):
    return round((max(values) - min(values)) / statistics.median(values), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libepik_amd.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--branches", type=int, default=9999)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)), flush=True)
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("strata_rate.py compares with a library built from the parent commit: --parent-lib PATH")
    from epik_amd import provenance
    rounds = {"this": [], "parent": []}
    for _ in range(args.rounds):                                                # alternating: this, parent, this, parent, ..
        rounds["this"].append(child(args, ""))
        rounds["parent"].append(child(args, os.path.abspath(args.parent_lib)))
    assert all(r["has_strata"] for r in rounds["this"]) and not any(r["has_strata"] for r in rounds["parent"])
    unstratified, stratified = {}, {}
    for name in rounds["parent"][0]["ms"]:
        ours, theirs = [r["ms"][name] for r in rounds["this"]], [r["ms"][name] for r in rounds["parent"]]
        unstratified[name] = {"this_ms": ours, "parent_ms": theirs, "this_over_parent": round(statistics.median(ours) / statistics.median(theirs), 4),
                              "spread_this": spread(ours), "spread_parent": spread(theirs)}
    for name in rounds["this"][0]["ms"]:
        if name.endswith("_none"):
            continue
        base = name.rsplit("_", 1)[0] + "_none"
        ours, theirs = [r["ms"][name] for r in rounds["this"]], [r["ms"][base] for r in rounds["parent"]]
        stratified[name] = {"this_ms": ours, "over_parent_unstratified": round(statistics.median(ours) / statistics.median(theirs), 3)}
    result = {"tool": "strata_rate", "provenance": provenance.summary(), "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
              "num_samples": args.samples, "num_branches": args.branches, "groups": 4, "unstratified": unstratified, "stratified": stratified}
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
