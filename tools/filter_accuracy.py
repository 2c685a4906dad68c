#!/usr/bin/env python3
"""What the informativeness filters keep of placement accuracy when --mu cuts the database: runs without a GPU, on the
host mirrors (ancestral reconstruction, builder, ranking) and the CPU oracle.

Two references: the tree of the end-to-end tests (24 leaves, 160 sites, k = 6) and a tree of 200 leaves (400 sites,
k = 8), each with an alignment evolved along it.  Reads are cut from the leaves' sequences; for every filter and every mu the
database file is written in that filter's order, read back with that mu, and the reads are placed by the oracle.  Reported:
the share of reads placed first on their own leaf's branch.  Writes profiles/filter_accuracy.json.

    python tools/filter_accuracy.py [--threads 16] [--out profiles/filter_accuracy.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epik_amd import ancestral, build, dbfile, filters, newick, synth  # noqa: E402

MUS = (1.0, 0.5, 0.25, 0.1)
MODEL = "GTR{1.2/3.1/0.8/1.1/3.4/1.0}+FC+G4{0.8}"
CASES = (dict(name="leaves24", leaves=24, sites=160, k=6, read_length=60, reads_per_leaf=8, seed=31),
         dict(name="leaves200", leaves=200, sites=400, k=8, read_length=100, reads_per_leaf=4, seed=57))


def evolved_alignment(tree, sites, rng):
    """A sequence per node: the root's is random, a child's its parent's with every site redrawn with probability
    min(0.6, 3 x branch length)."""
    seqs = np.zeros((tree.num_nodes, sites), dtype=np.int64)
    seqs[tree.num_nodes - 1] = rng.integers(0, 4, size=sites)
    for v in range(tree.num_nodes - 2, -1, -1):
        redraw = rng.random(sites) < min(0.6, 3.0 * tree.branch_length[v])
        seqs[v] = np.where(redraw, rng.integers(0, 4, size=sites), seqs[tree.parent[v]])
    return seqs


def run_case(case, threads, folder):
    from oracle import oracle
    rng = np.random.default_rng(case["seed"])
    tree = synth.make_tree(case["leaves"], seed=case["seed"])
    seqs = evolved_alignment(tree, case["sites"], rng)
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)
    leaves = [i for i in range(tree.num_nodes) if tree.children[i, 0] < 0]
    rows = {tree.labels[i]: chars[seqs[i]].tobytes().decode() for i in leaves}
    ref = newick.parse(tree.newick())
    masks = ancestral.leaf_masks(ref, rows, "nucl")
    parsed = ancestral.Model.parse(MODEL, "nucl").resolve(None, masks)
    weights, p_full, p_half, p_pend = parsed.tables(ref)
    t0 = time.time()
    post, branch_of, _ = ancestral.posteriors_host(ancestral.tree_parent(ref), 4, weights, parsed.freqs, p_full, p_half, p_pend, masks, "both",
                                                   num_threads=threads)
    db = build.build_host("nucl", case["k"], tree.num_nodes, build.logp_from_posteriors(post), branch_of, omega=1.5, num_threads=threads)
    built_s = time.time() - t0
    reads, home = [], []
    for i in leaves:
        for at in rng.integers(0, case["sites"] - case["read_length"] + 1, size=case["reads_per_leaf"]):
            reads.append(chars[seqs[i, at:at + case["read_length"]]].tobytes().decode())
            home.append(i)
    data, offs = synth.pack_reads(reads)
    home = np.array(home)
    result = dict(name=case["name"], leaves=case["leaves"], sites=case["sites"], k=case["k"], reads=len(reads), read_length=case["read_length"],
                  num_keys=int(len(db.keys)), num_entries=int(db.num_entries), build_seconds=round(built_s, 2), accuracy={}, entries_loaded={})
    for name in filters.FILTERS:
        _, order = filters.rank_host(db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, name, seed=1, num_threads=threads)
        path = os.path.join(folder, f"{case['name']}_{name}.ekdb")
        dbfile.write_db(path, db, tree.newick(), order=order)
        result["accuracy"][name], result["entries_loaded"][name] = {}, {}
        for mu in MUS:
            cut, _ = dbfile.read_db(path, mu=mu)
            o_rows, o_n, _ = oracle.Oracle.from_synth(cut).place(data, offs, num_threads=0)
            hit = (o_n > 0) & (o_rows[:, 0]["branch"] == home)
            result["accuracy"][name][str(mu)] = round(float(hit.mean()), 4)
            result["entries_loaded"][name][str(mu)] = int(cut.num_entries)
            print(f"{case['name']} {name:6s} mu={mu:<4} own-branch first: {hit.mean():.4f} ({int(cut.num_entries)} phylo-k-mers loaded)", flush=True)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_accuracy.json"))
    ap.add_argument("--cases", default=",".join(c["name"] for c in CASES))
    args = ap.parse_args()
    from oracle import oracle
    oracle.build()
    with tempfile.TemporaryDirectory() as folder:
        results = [run_case(c, args.threads, folder) for c in CASES if c["name"] in args.cases.split(",")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(tool="tools/filter_accuracy.py", model=MODEL, omega=1.5, mus=list(MUS), filters=list(filters.FILTERS),
                       measure="share of reads placed first on their own leaf's branch (CPU oracle on read_db(mu) of the file)",
                       cases=results), fh, indent=1)
        fh.write("\n")
    print(args.out)


if __name__ == "__main__":
    main()
