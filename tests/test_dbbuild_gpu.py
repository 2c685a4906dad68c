"""The database builder on the GPU (epik_amd_builder_*; epik_amd.build.Builder): every case of test_dbbuild_cpu.py
through the device builder, bytes equal to the host mirror's; the same bytes whatever the chunks, with a workspace so
small that `add` has to split a chunk by itself, and through the device-pointer entry; the refusals of a builder, its
store unchanged after each; and a database built from forged posteriors of a tree that places reads cut from a branch's
sequence on that branch -- in memory, and from files through `epik.py build` and `epik.py place`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import build, capi, dbfile, jplace, jplace_diff, synth
from test_dbbuild_cpu import (ALL_CASES, CHUNKING_CASE, EPIK_PY, ROOT, forged_build_input, get_case, run_host, same_db, well_formed,
                              write_ar_files)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"


_HOST = {}


def host_of(name):
    """The host mirror's database of a case, computed once."""
    if name not in _HOST:
        _HOST[name] = run_host(get_case(name))
    return _HOST[name]


def builder_for(case, **kw):
    return build.Builder(case["states"], case["k"], case["N"], log_thr=case["log_thr"], **kw)


@pytest.mark.parametrize("name", ALL_CASES)
def test_device_equals_host_mirror(name):
    case = get_case(name)
    with builder_for(case) as b:
        b.add(case["logp"], case["branch_of"])
        db = b.finish()
    same_db(db, host_of(name))
    well_formed(db)


def test_threshold_seam_on_the_device():
    case = get_case("nucl-k5-L63-G3")
    lowest = host_of("nucl-k5-L63-G3").values["score"].min()
    for thr in (np.float32(lowest), np.nextafter(np.float32(lowest), np.float32(0))):
        case["log_thr"] = thr
        with builder_for(case) as b:
            b.add(case["logp"], case["branch_of"])
            same_db(b.finish(), run_host(case))


def test_chunking_cannot_change_a_bit():
    case = get_case(CHUNKING_CASE)
    logp, branch_of = case["logp"], case["branch_of"]
    G = logp.shape[0]
    want = host_of(CHUNKING_CASE)
    for step in (G, 1, 7):
        with builder_for(case) as b:
            for g in range(0, G, step):
                b.add(logp[g:g + step], branch_of[g:g + step])
            db = b.finish()
            assert b.num_splits == 0
        same_db(db, want)
    # a workspace the chunk's tuples do not fit: `add` splits the chunk by ghost nodes and goes on
    with builder_for(case, workspace_bytes=3 << 20) as b:
        b.add(logp, branch_of)
        db = b.finish()
        assert b.num_splits > 0
    same_db(db, want)
    # ... and one that a single ghost node does not fit is refused by name
    with builder_for(case, workspace_bytes=8 << 10) as b:
        with pytest.raises(capi.EpikAmdError, match=r"ghost node 0 of the chunk needs a workspace of \d+ bytes, the builder has 8192"):
            b.add(logp, branch_of)


def test_finish_may_be_followed_by_more_chunks():
    case = get_case("nucl-k5-L65-G3")
    with builder_for(case) as b:
        b.add(case["logp"][:1], case["branch_of"][:1])
        first = b.finish()
        b.add(case["logp"][1:], case["branch_of"][1:])
        same_db(b.finish(), host_of("nucl-k5-L65-G3"))
    assert 0 < first.num_entries < host_of("nucl-k5-L65-G3").num_entries


@pytest.mark.parametrize("name", ["nucl-k5-L65-G3", "amino-k3-L63-G3", "special"])
def test_device_entry(name):
    import torch
    case = get_case(name)
    d_logp = torch.from_numpy(case["logp"]).cuda()
    d_branch = torch.from_numpy(case["branch_of"].view(np.int32)).cuda()
    with builder_for(case) as b:
        b.add_device(d_logp, d_branch)
        same_db(b.finish(), host_of(name))


def test_builder_refusals_leave_the_store_alone():
    import torch
    case = get_case("nucl-k5-L65-G3")
    logp, branch_of = case["logp"], case["branch_of"]
    want = host_of("nucl-k5-L65-G3")
    bad_nan, bad_pos, bad_branch = logp.copy(), logp.copy(), branch_of.copy()
    bad_nan[2, 17, 3] = np.nan
    bad_pos[1, 0, 1] = np.float32(1e-3)
    bad_branch[1] = case["N"]
    refusals = [
        (bad_nan, branch_of, r"ghost node 2, site 17, state 3: logp is NaN"),
        (bad_pos, branch_of, r"ghost node 1, site 0, state 1: logp is above 0"),
        (logp, bad_branch, r"branch_of\[1\] = 7 is no branch of a tree of 7"),
        (logp[:, :4], branch_of, r"L = 4 sites hold no window of k = 5"),
        (logp[:, :64], branch_of, r"L = 64 differs from the first chunk's L = 65"),
    ]
    with builder_for(case) as b:
        b.add(logp, branch_of)
        for chunk, branches, message in refusals:
            with pytest.raises(capi.EpikAmdError, match=message) as info:
                b.add(np.ascontiguousarray(chunk), branches)
            assert info.value.code == capi.ERR_INVALID
            with pytest.raises(capi.EpikAmdError, match=message):
                b.add_device(torch.from_numpy(np.ascontiguousarray(chunk)).cuda(), torch.from_numpy(branches.view(np.int32).copy()).cuda())
            same_db(b.finish(), want)
        b.add(logp[:0], branch_of[:0])  # no ghost node: a valid no-op
        same_db(b.finish(), want)
    for kw, message in ((dict(k=16), r"k = 16 is outside \[2, 15\] for sigma = 4"), (dict(k=1), r"k = 1 is outside"),
                        (dict(states="amino", k=8), r"k = 8 is outside \[2, 7\] for sigma = 20"), (dict(N=0), r"at least one branch"),
                        (dict(log_thr=np.float32(0.5)), r"log_thr must be a number that is at most 0")):
        args = dict(states="nucl", k=5, N=7, log_thr=None)
        args.update(kw)
        with pytest.raises(capi.EpikAmdError, match=message):
            builder_for(args)


def test_from_posteriors_to_placements(tmp_path):
    """A tree of 40 leaves, a random sequence per branch, ghost posteriors of 0.97 on it: the database built on the device
    places every read cut from a branch's sequence on that branch (checked on the CPU in test_dbbuild_cpu.py); the same
    input written to files and built by `epik.py build` gives the same database, and `epik.py place` on it the jplace of
    the placement in memory."""
    from epik_amd.placer import PlacedCollection, PlacedSequence, Placement, Placer, pendant_lengths
    tree, post, reads, source = forged_build_input()
    branches = post.shape[0]
    logp = build.logp_from_posteriors(np.concatenate([post, post]))
    branch_of = np.tile(np.arange(branches), 2).astype(np.uint32)
    with build.Builder("nucl", 8, tree.num_nodes, omega=1.5) as b:
        b.add(logp, branch_of)
        db = b.finish()
    same_db(db, build.build_host("nucl", 8, tree.num_nodes, logp, branch_of, omega=1.5, num_threads=4))
    seq_map = {}
    for i, s in enumerate(reads):
        seq_map.setdefault(s, []).append(f"read_{i}")
    unique = list(seq_map)
    home = {s: int(source[i]) for i, s in enumerate(reads)}
    data, offs = synth.pack_reads(unique)
    with Placer.from_synth(db, tree, device=0) as pl:
        rows, n_rows, counts = pl.place_packed(data, offs)
    assert np.all(n_rows >= 1)
    assert np.array_equal(rows[:, 0]["branch"], np.array([home[s] for s in unique]))

    # from files
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tree_path, probs, ar_tree = write_ar_files(tmp_path, tree, post, reroot_at="P5")
    db_path = str(tmp_path / "built.ekdb")
    run = subprocess.run([sys.executable, EPIK_PY, "build", "-t", tree_path, "--ar-probs", probs, "--ar-tree", ar_tree, "-s", "nucl",
                          "-k", "8", "--omega", "1.5", "--chunk", "50", "-o", db_path], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"{db.keys.shape[0]} k-mers, {db.num_entries} phylo-k-mers from {2 * branches} ghost nodes" in run.stdout
    got, text = dbfile.read_db(db_path)
    dense = db.densified()
    assert text == tree.newick() and got.num_branches == tree.num_nodes
    assert np.array_equal(got.offsets, dense.offsets) and got.values.tobytes() == dense.values.tobytes()

    fasta = str(tmp_path / "q.fasta")
    with open(fasta, "w") as fh:
        for i, s in enumerate(reads):
            fh.write(f">read_{i}\n{s}\n")
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    run = subprocess.run([sys.executable, EPIK_PY, "place", "-i", db_path, "-o", str(out_dir), fasta], capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert f"Placed {len(reads)} sequences." in run.stdout
    distal, pendant = pendant_lengths(tree.branch_length, tree.subtree_num_nodes, tree.subtree_total_length)
    placed = []
    for i, s in enumerate(unique):
        mine = []
        for r in range(n_rows[i]):
            br, c = int(rows[i, r]["branch"]), int(counts[i, r])
            mine.append(Placement(br, float(rows[i, r]["score"]), float(rows[i, r]["lwr"]), c, float(distal[br]) if c else 0.0,
                                  float(pendant[br]) if c else 0.0))
        placed.append(PlacedSequence(s, mine))
    ref_path = str(tmp_path / "memory.jplace")
    jplace.write_jplace(ref_path, PlacedCollection(seq_map, placed), "memory", tree.newick(jplace=True))
    from_files, in_memory = jplace.read_jplace(str(out_dir / "placements_q.fasta.jplace")), jplace.read_jplace(ref_path)
    assert set(from_files) == set(in_memory) == {f"read_{i}" for i in range(len(reads))}
    assert jplace_diff.diff_strict(from_files, in_memory) == []
