"""Ranking phylo-k-mers by informativeness on the GPU (epik_amd_filter_rank_device, epik_amd_filter_rank,
epik_amd_builder_rank; epik_amd.filters): bytes equal to the host mirror's -- the forged databases of test_filter_cpu.py
into poisoned buffers on a stream of its own, key counts around the tile and the workgroup, a database whose tiles mix
one-entry keys with long lists and that the grid strides over, every lane-per-key length beside a longer list; the
builder's own arrays after chunked adds; and tree + alignment through `epik.py reconstruct --filter mif0`, `epik.py place
--mu 0.5` and `epik.py rank`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import build, capi, dbfile, filters, jplace, jplace_diff, synth
from epik_amd.synth import PKDB_VALUE
from test_ancestral_gpu import evolved_alignment
from test_filter_cpu import BRANCH_COUNTS, EPIK_PY, FINITE_THR, ROOT, forge_lists, get_forged, same_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"


def rank_on_stream(num_branches, log_thr, keys, offsets, values, name, seed):
    """rank_device on tensors of the device, on a stream of its own, into buffers full of 0xA5."""
    import torch
    stream = torch.cuda.Stream()
    d_keys = torch.from_numpy(keys.view(np.int32).copy()).cuda()
    d_offsets = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
    d_values = torch.from_numpy(np.ascontiguousarray(values).view(np.int64).copy()).cuda()
    K = len(keys)
    d_value = torch.full((K,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda").view(torch.float64)
    d_order = torch.full((K,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    filters.rank_device(num_branches, log_thr, d_keys, d_offsets, d_values, name, seed=seed, d_value=d_value, d_order=d_order,
                        stream=stream.cuda_stream)
    return d_value.cpu().numpy(), d_order.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("log_thr", [FINITE_THR, np.float32(-np.inf)], ids=["thr", "thr-inf"])
@pytest.mark.parametrize("num_branches", BRANCH_COUNTS)
def test_device_equals_host_mirror(num_branches, log_thr):
    keys, offsets, values = get_forged(num_branches, log_thr)
    for name in filters.FILTERS:
        want = filters.rank_host(num_branches, log_thr, keys, offsets, values, name, seed=77)
        assert same_bytes(rank_on_stream(num_branches, log_thr, keys, offsets, values, name, 77), want), name
        assert same_bytes(filters.rank(num_branches, log_thr, keys, offsets, values, name, seed=77), want), name


@pytest.mark.parametrize("num_keys", [1, 63, 64, 65, 255, 256, 257])
def test_key_counts_around_the_tile_and_the_workgroup(num_keys):
    rng = np.random.default_rng(num_keys)
    lengths = rng.choice([1, 2, 3, 4, 5, 9, 70, 130], size=num_keys)
    lengths[-1] = 130                                   # the last key of the last tile has a long list
    keys, offsets, values = forge_lists(lengths, 200, FINITE_THR, rng)
    for name in filters.FILTERS:
        want = filters.rank_host(200, FINITE_THR, keys, offsets, values, name, seed=5)
        assert same_bytes(rank_on_stream(200, FINITE_THR, keys, offsets, values, name, 5), want), name


def test_tiles_that_mix_short_and_long_lists_under_the_grid_stride():
    """About 70 000 keys in 1 094 tiles on 274 workgroups, one tile a wave: most keys have one entry, every tile a few lists
    longer than 64 x 4, and scores with many ties.  (The grid's own stride begins above 32 768 tiles; the second sweep is
    test_build_seams_gpu.py's.)"""
    rng = np.random.default_rng(17)
    K, N = 70001, 400
    lengths = np.ones(K, dtype=np.int64)
    long_at = np.flatnonzero(rng.random(K) < 0.04)
    lengths[long_at] = rng.integers(257, 391, size=len(long_at))
    lengths[np.flatnonzero(rng.random(K) < 0.1)] = 2
    keys, offsets, values = forge_lists(lengths, N, FINITE_THR, rng)
    values["score"][rng.random(len(values)) < 0.3] = np.float32(-2.0)
    assert (lengths > 256).sum() > 2000 and (lengths == 1).sum() > 50000
    for name in filters.FILTERS:
        want = filters.rank_host(N, FINITE_THR, keys, offsets, values, name, seed=9, num_threads=16)
        assert same_bytes(rank_on_stream(N, FINITE_THR, keys, offsets, values, name, 9), want), name


def test_every_lane_per_key_length_beside_a_longer_list():
    rng = np.random.default_rng(23)
    lengths = np.array([1, 5, 2, 5, 3, 5, 4, 5, 5, 1, 2, 3, 4, 64, 4, 3, 2, 1], dtype=np.int64)
    keys, offsets, values = forge_lists(lengths, 90, FINITE_THR, rng)
    values["score"][:] = -(rng.random(len(values)) * 3).astype(np.float32)      # no ties, no zeros: every term counts
    for name in filters.FILTERS:
        want = filters.rank_host(90, FINITE_THR, keys, offsets, values, name, seed=1)
        assert same_bytes(filters.rank(90, FINITE_THR, keys, offsets, values, name, seed=1), want), name
        assert same_bytes(want, filters.rank_numpy(90, FINITE_THR, keys, offsets, values, name, seed=1)), name


def test_device_refusals():
    keys, offsets, values = (a.copy() for a in get_forged(65, FINITE_THR))

    def refused(message, **kw):
        args = dict(num_branches=65, log_thr=FINITE_THR, keys=keys, offsets=offsets, values=values, filter=1)
        args.update(kw)
        with pytest.raises(capi.EpikAmdError, match=message) as info:
            rank_on_stream(args["num_branches"], args["log_thr"], args["keys"], args["offsets"], args["values"], args["filter"], 0)
        assert info.value.code == capi.ERR_INVALID

    refused("unknown filter 3", filter=3)
    bad = values.copy()
    bad["score"][40] = np.nan
    bad["score"][300] = 0.25
    bad["branch"][7] = 65
    refused(r"values\[40\]\.score = nan is a NaN or above 0", values=bad)
    bad["score"][40] = -1.0
    refused(r"values\[300\]\.score = 0\.25 is a NaN or above 0", values=bad, filter=0)
    bad["score"][300] = -1.0
    refused(r"values\[7\]\.branch = 65 is not below num_branches = 65", values=bad, filter=2)
    wrong = offsets.copy()
    wrong[9] = wrong[8] - 1
    refused(r"offsets\[9\] = \d+ is below offsets\[8\]", offsets=wrong)
    wrong = offsets.copy()
    wrong[9] = wrong[-1] + 5                       # beyond the last one: nothing is read through it
    refused(r"offsets\[9\] = \d+ is above the last one", offsets=wrong)
    empty = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, PKDB_VALUE))
    value, order = filters.rank(5, FINITE_THR, *empty, "mif0")
    assert value.shape == (0,) and order.shape == (0,)


def test_builder_rank_after_chunked_adds():
    """Builder.rank on the builder's own device arrays: rank_host on builder_copy's arrays, whatever the chunks, and again
    after more chunks and a second finish."""
    rng = np.random.default_rng(41)
    N, k, G, L = 33, 6, 48, 40
    post = rng.dirichlet(np.full(4, 0.25), size=(G, L)).astype(np.float32)
    logp, branch_of = build.logp_from_posteriors(post), rng.integers(0, N, size=G).astype(np.uint32)

    def ranked(builder):
        db = builder.finish()
        got = {name: builder.rank(name, seed=4) for name in filters.FILTERS}
        for name in filters.FILTERS:
            want = filters.rank_host(N, db.log_threshold, db.keys, db.offsets, db.values, name, seed=4)
            assert same_bytes(got[name], want), name
        return db, got

    with build.Builder("nucl", k, N, omega=1.5) as whole, build.Builder("nucl", k, N, omega=1.5) as chunked:
        whole.add(logp[:32], branch_of[:32])
        for g in range(0, 32, 5):
            chunked.add(logp[g:min(g + 5, 32)], branch_of[g:min(g + 5, 32)])
        db_a, got_a = ranked(whole)
        db_b, got_b = ranked(chunked)
        assert db_a.values.tobytes() == db_b.values.tobytes() and len(db_a.keys) > 300
        for name in filters.FILTERS:
            assert same_bytes(got_a[name], got_b[name])
        assert not np.array_equal(got_a["mif0"][1], got_a["best"][1])
        whole.add(logp[32:], branch_of[32:])
        for g in range(32, G, 7):
            chunked.add(logp[g:g + 7], branch_of[g:g + 7])
        db_a2, got_a2 = ranked(whole)
        db_b2, got_b2 = ranked(chunked)
        assert db_a2.num_entries > db_a.num_entries and db_a2.values.tobytes() == db_b2.values.tobytes()
        for name in filters.FILTERS:
            assert same_bytes(got_a2[name], got_b2[name])


def test_from_tree_and_alignment_to_placements_at_half_the_database(tmp_path):
    """`epik.py reconstruct --filter mif0` on the tree of test_ancestral_gpu.py (24 leaves, 160 sites, k = 6), then `epik.py
    place --mu 0.5`: the jplace of the oracle on read_db(mu = 0.5) of the same file; and `epik.py rank --filter mif0` on the
    `best` file gives the mif0 file's bytes."""
    from epik_amd.placer import PlacedCollection, PlacedSequence, Placement, pendant_lengths
    from oracle import oracle
    rng = np.random.default_rng(31)
    tree = synth.make_tree(24, seed=31)
    sites, k, read_length = 160, 6, 60
    seqs = evolved_alignment(tree, sites, rng)
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)
    leaves = [i for i in range(tree.num_nodes) if tree.children[i, 0] < 0]
    rows = {tree.labels[i]: chars[seqs[i]].tobytes().decode() for i in leaves}
    tree_path, fasta = str(tmp_path / "ref.nwk"), str(tmp_path / "ref.fasta")
    with open(tree_path, "w") as fh:
        fh.write(tree.newick() + "\n")
    with open(fasta, "w") as fh:
        for name, seq in rows.items():
            fh.write(f">{name}\n{seq}\n")
    model = "GTR{1.2/3.1/0.8/1.1/3.4/1.0}+FC+G4{0.8}"
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    paths = {name: str(tmp_path / f"{name}.ekdb") for name in ("best", "mif0", "reranked")}
    for name in ("best", "mif0"):
        run = subprocess.run([sys.executable, EPIK_PY, "reconstruct", "-t", tree_path, "-r", fasta, "--model", model, "-s", "nucl", "-k", str(k),
                              "--omega", "1.5", "--chunk", "20", "--filter", name, "-o", paths[name]], capture_output=True, text=True,
                             timeout=600)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    run = subprocess.run([sys.executable, EPIK_PY, "rank", "-i", paths["best"], "--filter", "mif0", "-o", paths["reranked"]],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    mif0_bytes = open(paths["mif0"], "rb").read()
    assert open(paths["reranked"], "rb").read() == mif0_bytes != open(paths["best"], "rb").read()
    # the file holds the keys in rank_numpy's mif0 order
    whole, text = dbfile.read_db(paths["mif0"])
    lens = np.diff(whole.offsets.astype(np.int64))
    keys = np.flatnonzero(lens).astype(np.uint32)
    offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens[keys])
    _, order = filters.rank_numpy(whole.num_branches, whole.log_threshold, keys, offsets, whole.values, "mif0")
    db, _ = dbfile.read_db(paths["mif0"], mu=0.5)
    kept = np.flatnonzero(np.diff(db.offsets.astype(np.int64)))
    assert set(kept.tolist()) == set(keys[order[:-(-len(keys) // 2)]].tolist()) and len(kept) < len(keys)

    reads = []
    for i in leaves:
        for at in rng.integers(0, sites - read_length + 1, size=8):
            reads.append(chars[seqs[i, at:at + read_length]].tobytes().decode())
    query = str(tmp_path / "q.fasta")
    with open(query, "w") as fh:
        for i, s in enumerate(reads):
            fh.write(f">read_{i}\n{s}\n")
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    run = subprocess.run([sys.executable, EPIK_PY, "place", "-i", paths["mif0"], "--mu", "0.5", "-o", str(out_dir), query], capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"Placed {len(reads)} sequences." in run.stdout

    seq_map = {}
    for i, s in enumerate(reads):
        seq_map.setdefault(s, []).append(f"read_{i}")
    unique = list(seq_map)
    data, offs = synth.pack_reads(unique)
    oracle.build()
    o_rows, o_n, o_counts = oracle.Oracle.from_synth(db).place(data, offs, num_threads=0)
    distal, pendant = pendant_lengths(tree.branch_length, tree.subtree_num_nodes, tree.subtree_total_length)
    placed = []
    for i, s in enumerate(unique):
        mine = []
        for r in range(o_n[i]):
            br, c = int(o_rows[i, r]["branch"]), int(o_counts[i, r])
            mine.append(Placement(br, float(o_rows[i, r]["score"]), float(o_rows[i, r]["lwr"]), c, float(distal[br]) if c else 0.0,
                                  float(pendant[br]) if c else 0.0))
        placed.append(PlacedSequence(s, mine))
    ref_path = str(tmp_path / "oracle.jplace")
    jplace.write_jplace(ref_path, PlacedCollection(seq_map, placed), "oracle", tree.newick(jplace=True))
    from_files, in_memory = jplace.read_jplace(str(out_dir / "placements_q.fasta.jplace")), jplace.read_jplace(ref_path)
    assert set(from_files) == set(in_memory) == {f"read_{i}" for i in range(len(reads))}
    assert jplace_diff.diff_strict(from_files, in_memory) == []
