#!/usr/bin/env python3
"""Cost of translated placement: epik_amd_placer_place_device on protein reads against
epik_amd_placer_place_frames_device on the nucleotide reads they were back-translated from (modes forward and both:
three or six frames per read, the translate and frame-select kernels around ONE placement of all frames), on
device-resident reads, timed with HIP events on one stream after warm-up.  Workload: the configs[3] shape (amino
k = 7, N = 999, the sparse database of tests/test_configs_gpu.py), 150 bp reads (50-residue proteins, a quarter of
their positions starting a k-mer of the database, random synonymous codons, half of them reverse-complemented).

    python tools/frame_rate.py [--reads 1048576] [--steps 10] [--warmup 3] [--out file.json]

Prints one JSON line: the median milliseconds of each call and their ratios.  Under
`rocprofv3 --kernel-trace --stats` the kernels' own shares show in the trace.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CODONS = {"A": "GCT GCC GCA GCG", "R": "CGT CGC CGA CGG AGA AGG", "N": "AAT AAC", "D": "GAT GAC", "C": "TGT TGC",
          "Q": "CAA CAG", "E": "GAA GAG", "G": "GGT GGC GGA GGG", "H": "CAT CAC", "I": "ATT ATC ATA", "L":
          "TTA TTG CTT CTC CTA CTG", "K": "AAA AAG", "M": "ATG", "F": "TTT TTC", "P": "CCT CCC CCA CCG", "S":
          "TCT TCC TCA TCG AGT AGC", "T": "ACT ACC ACA ACG", "W": "TGG", "Y": "TAT TAC", "V": "GTT GTC GTA GTG"}


def back_translate(pdata: np.ndarray, n: int, residues: int, seed: int) -> np.ndarray:
    """uint8[n * residues] protein letters -> uint8[n * 3 * residues] nucleotides, every other read reverse-complemented."""
    rng = np.random.default_rng(seed)
    table = np.zeros((256, 6, 3), dtype=np.uint8)
    choices = np.ones(256, dtype=np.int64)
    for aa, codons in CODONS.items():
        cs = codons.split()
        choices[ord(aa)] = len(cs)
        for j in range(6):
            table[ord(aa), j] = np.frombuffer(cs[j % len(cs)].encode(), dtype=np.uint8)
    pick = (rng.random(pdata.shape[0]) * choices[pdata]).astype(np.int64)
    nt = table[pdata, pick].reshape(n, 3 * residues)
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    nt[1::2] = comp[nt[1::2, ::-1]]
    return nt.reshape(-1).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch  # (first: its HIP runtime before libepik_amd's, capi.check_hip_runtime)
    from epik_amd import capi, synth
    from epik_amd.placer import Placer
    n, residues = args.reads, args.read_length // 3
    tree = synth.make_tree(500, seed=42)
    db = synth.make_sparse_db(tree.num_nodes, states="amino", kmer_size=7, p_present=0.0026, seed=43)
    pdata, poffs = synth.reads_hitting(db, n, residues, hit_rate=0.25, seed=46)
    ndata = back_translate(pdata, n, residues, seed=47)
    noffs = np.arange(n + 1, dtype=np.uint64) * np.uint64(3 * residues)
    dev = torch.device("cuda", 0)
    with Placer.from_synth(db) as pl:
        keep = pl.keep_at_most
        pl.choose_counts(residues)
        d_prot = torch.from_numpy(pdata).to(dev)
        d_poffs = torch.from_numpy(poffs.view(np.int64)).to(dev)
        d_nt = torch.from_numpy(ndata).to(dev)
        d_noffs = torch.from_numpy(noffs.view(np.int64)).to(dev)
        d_rows = torch.zeros(n * keep * 2, dtype=torch.float64, device=dev)
        d_n = torch.zeros(n, dtype=torch.int32, device=dev)
        d_counts = torch.zeros(n * keep, dtype=torch.int32, device=dev)
        d_frame = torch.zeros(n, dtype=torch.uint8, device=dev)
        ws = pl.frame_workspace_bytes(n, int(noffs[-1]), capi.FRAMES_BOTH)
        d_ws = torch.empty(ws, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream()
        s = stream.cuda_stream

        def protein():
            pl.place_device(d_prot.data_ptr(), d_poffs.data_ptr(), n, d_rows.data_ptr(), d_n.data_ptr(),
                            d_counts.data_ptr(), s)

        def frames(mode):
            return lambda: pl.place_frames_device(d_nt.data_ptr(), d_noffs.data_ptr(), n, mode, d_ws.data_ptr(), ws,
                                                  d_rows.data_ptr(), d_n.data_ptr(), d_counts.data_ptr(),
                                                  d_frame.data_ptr(), s)

        times, right = {}, {}
        for name, fn in (("protein", protein), ("forward", frames(capi.FRAMES_FORWARD)),
                         ("both", frames(capi.FRAMES_BOTH))):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.steps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms.append(a.elapsed_time(b))
            times[name] = ms
            if name == "both":  # (the generating frame: +1, or -1 for the reverse-complemented half)
                right[name] = float((d_frame.cpu().numpy() == np.where(np.arange(n) % 2 == 1, 3, 0)).mean())
    med = {k: statistics.median(v) for k, v in times.items()}
    line = {"workload": f"amino k=7 N={tree.num_nodes} (configs[3] shape), {n} x {args.read_length} bp reads, "
                        f"device-resident", "steps": args.steps, "warmup": args.warmup,
            "protein_ms": med["protein"], "forward_ms": med["forward"], "both_ms": med["both"],
            "forward_reads_per_s": n / med["forward"] * 1e3, "both_reads_per_s": n / med["both"] * 1e3,
            "forward_over_protein": med["forward"] / med["protein"], "both_over_protein": med["both"] / med["protein"],
            "reads_in_generating_frame_both": right["both"], "ms_all": times}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
