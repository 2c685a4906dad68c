"""The database builder without a GPU (include/epik_amd.h, "Building a phylo-k-mer database"): the host mirror
epik_amd_build_host against build_numpy, an independent restatement of the rule -- keys, offsets and value bytes equal --
on the shapes where the enumeration can go wrong, at the threshold's seam, with everything and nothing surviving, with
p = 0 and p = 1, with the same k-mer met several times, and on float32 values whose sum depends on the order of the
additions; every refusal of the host entry with its message; then the file side: newick.py's numbering, `epik.py extend`,
the posterior reader, the ghost nodes found in a re-rooted tree, `epik.py build`'s refusals, and the end-to-end claim of
test_dbbuild_gpu.py checked with the host mirror and the CPU oracle.  The cases are shared with test_dbbuild_gpu.py, which
runs the same inputs through the device builder."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epik_amd import alphabet, build, capi  # noqa: E402


def same_db(a, b):
    """Keys, offsets and the bytes of the values."""
    assert a.keys.dtype == np.uint32 and b.keys.dtype == np.uint32 and a.offsets.dtype == np.uint64 and b.offsets.dtype == np.uint64
    assert np.array_equal(a.keys, b.keys), "keys differ"
    assert np.array_equal(a.offsets, b.offsets), "offsets differ"
    assert a.values.tobytes() == b.values.tobytes(), "value bytes differ"


def well_formed(db):
    assert db.offsets.shape[0] == db.keys.shape[0] + 1 and int(db.offsets[0]) == 0 and int(db.offsets[-1]) == db.values.shape[0]
    assert np.all(np.diff(db.keys.astype(np.int64)) > 0) and np.all(np.diff(db.offsets.astype(np.int64)) > 0)
    for i in range(min(len(db.keys), 200)):
        br = db.values["branch"][int(db.offsets[i]):int(db.offsets[i + 1])].astype(np.int64)
        assert np.all(np.diff(br) > 0) and br.max() < db.num_branches
    assert np.all(db.values["score"] >= db.log_threshold)
    assert not np.any((db.values["score"].view(np.uint32)) == 0x80000000), "-0.0 among the scores"


def peaked_posteriors(rng, G, L, sigma, alpha=0.3):
    """Posteriors with one or two likely states a site, four decimals (as a posterior file prints them), rows summing to about 1."""
    p = rng.dirichlet(np.full(sigma, alpha), size=(G, L))
    return np.round(p, 4).astype(np.float32)


def spread_posteriors(rng, G, L, sigma, top=0.9):
    """`top` on one state of every site, the rest spread unevenly over the others."""
    rest = rng.dirichlet(np.ones(sigma - 1), size=(G, L)) * (1.0 - top)
    main = rng.integers(0, sigma, size=(G, L))
    idx = np.arange(sigma)[None, None, :]
    source = np.clip(np.where(idx < main[..., None], idx, idx - 1), 0, sigma - 2)  # the rest's slot of every other state
    out = np.take_along_axis(rest, source, axis=2)
    out[np.broadcast_to(idx, out.shape) == main[..., None]] = top
    return np.round(out, 5).astype(np.float32)


def make_case(states, k, L, G, N, seed, kind="peaked"):
    rng = np.random.default_rng(seed)
    sigma = alphabet.alphabet_size(states)
    p = peaked_posteriors(rng, G, L, sigma) if kind == "peaked" else spread_posteriors(rng, G, L, sigma)
    logp = build.logp_from_posteriors(p)
    branch_of = rng.integers(0, N, size=G).astype(np.uint32)  # repeats, any order
    if G >= 3:
        branch_of[0], branch_of[1], branch_of[2] = N - 1, 0, N - 1
    return dict(states=states, k=k, N=N, logp=logp, branch_of=branch_of, log_thr=None)


# (id, states, k, L, G, N, kind): L in {k, k + 1, 63, 64, 65, 130}, G in {1, 3, 130}
SHAPES = [
    ("nucl-k2-L2-G1", "nucl", 2, 2, 1, 3, "peaked"),
    ("nucl-k2-L3-G3", "nucl", 2, 3, 3, 5, "peaked"),
    ("nucl-k2-L130-G130", "nucl", 2, 130, 130, 11, "peaked"),
    ("nucl-k5-L5-G3", "nucl", 5, 5, 3, 5, "peaked"),
    ("nucl-k5-L6-G1", "nucl", 5, 6, 1, 1, "peaked"),
    ("nucl-k5-L63-G3", "nucl", 5, 63, 3, 7, "peaked"),
    ("nucl-k5-L64-G3", "nucl", 5, 64, 3, 7, "peaked"),
    ("nucl-k5-L65-G3", "nucl", 5, 65, 3, 7, "peaked"),
    ("nucl-k5-L130-G130", "nucl", 5, 130, 130, 37, "peaked"),
    ("nucl-k8-L8-G3", "nucl", 8, 8, 3, 4, "peaked"),
    ("nucl-k8-L9-G1", "nucl", 8, 9, 1, 2, "peaked"),
    ("nucl-k8-L72-G3", "nucl", 8, 72, 3, 300, "peaked"),
    ("amino-k2-L2-G130", "amino", 2, 2, 130, 70000, "peaked"),
    ("amino-k2-L65-G3", "amino", 2, 65, 3, 9, "peaked"),
    ("amino-k3-L4-G1", "amino", 3, 4, 1, 2, "peaked"),
    ("amino-k3-L63-G3", "amino", 3, 63, 3, 9, "peaked"),
    ("amino-k3-L130-G3", "amino", 3, 130, 3, 9, "peaked"),
    ("amino-k7-L8-G3-frontier", "amino", 7, 8, 3, 5, "spread"),
    ("amino-k7-L7-G1-frontier", "amino", 7, 7, 1, 5, "spread"),
]
CHUNKING_CASE = "nucl-k5-L130-G130"


def shape_case(name):
    for i, (cid, states, k, L, G, N, kind) in enumerate(SHAPES):
        if cid == name:
            return make_case(states, k, L, G, N, seed=1000 + i, kind=kind)
    raise KeyError(name)


def everything_case():
    """k = 6, sigma = 4, log_thr = -1e30, L = 70, G = 2: 4 096 survivors a window."""
    case = make_case("nucl", 6, 70, 2, 3, seed=77)
    case["branch_of"] = np.array([2, 0], dtype=np.uint32)
    case["log_thr"] = np.float32(-1e30)
    return case


def nothing_case():
    """Uniform posteriors at omega = 1.5: 0.25 a letter against a threshold of 0.375 a letter."""
    logp = build.logp_from_posteriors(np.full((3, 40, 4), 0.25, dtype=np.float32))
    return dict(states="nucl", k=6, N=4, logp=logp, branch_of=np.array([1, 3, 1], dtype=np.uint32), log_thr=None)


def special_case(negative_zero=False):
    """Sites with p = 1 on one state and p = 0 elsewhere between ordinary sites: logp holds +0.0 and -inf; runs of k
    such sites give a score of +0.0.  negative_zero: the zeros handed in as -0.0."""
    rng = np.random.default_rng(5)
    p = peaked_posteriors(rng, 3, 40, 4)
    hot = np.zeros((40,), dtype=bool)
    hot[3:12] = hot[20] = hot[30:33] = True
    onehot = np.eye(4, dtype=np.float32)[rng.integers(0, 4, size=(3, 40))]
    p[:, hot] = onehot[:, hot]
    logp = build.logp_from_posteriors(p)
    assert np.isneginf(logp).any() and (logp == 0).any()
    if negative_zero:
        logp = np.where(logp == 0, np.float32(-0.0), logp).astype(np.float32)
        assert (logp.view(np.uint32) == 0x80000000).any()
    return dict(states="nucl", k=4, N=6, logp=logp, branch_of=np.array([5, 2, 5], dtype=np.uint32), log_thr=None)


def periodic_case():
    """Forged periodic posteriors: the k-mer ACGTA is met at windows 0, 4 and 8 of ghost nodes 0 and 1, same branch, under
    different peaks; ghost node 2 carries it on another branch."""
    k, L = 5, 15
    letters = np.arange(L) % 4
    p = np.full((3, L, 4), 0.0, dtype=np.float32)
    peaks = np.array([[0.91] * 5 + [0.97] * 5 + [0.85] * 5, [0.94] * 15, [0.88] * 15], dtype=np.float32)
    for g in range(3):
        p[g] = ((1.0 - peaks[g]) / 3.0)[:, None]
        p[g, np.arange(L), letters] = peaks[g]
    # period 4 letters and k = 5: window w holds letters w .. w + 4 mod 4, so windows 0, 4 and 8 hold the same k-mer
    return dict(states="nucl", k=k, N=4, logp=build.logp_from_posteriors(p), branch_of=np.array([1, 1, 3], dtype=np.uint32),
                log_thr=None, peaks=peaks, letters=letters)


def rounding_case():
    """Random float32 logp (not the logarithm of anything printed): sums that depend on the order of the additions."""
    rng = np.random.default_rng(9)
    logp = (-rng.random((3, 40, 4)) * rng.choice([0.05, 0.4, 3.0], size=(3, 40, 4))).astype(np.float32)
    return dict(states="nucl", k=8, N=5, logp=logp, branch_of=np.array([4, 0, 4], dtype=np.uint32), log_thr=None)


SPECIAL = {"everything": everything_case, "nothing": nothing_case, "special": special_case,
           "special-negative-zero": lambda: special_case(True), "periodic": periodic_case, "rounding": rounding_case}
ALL_CASES = [s[0] for s in SHAPES] + sorted(SPECIAL)


def get_case(name):
    return SPECIAL[name]() if name in SPECIAL else shape_case(name)


def run_host(case, **kw):
    return build.build_host(case["states"], case["k"], case["N"], case["logp"], case["branch_of"], log_thr=case["log_thr"], **kw)


def run_numpy(case):
    return build.build_numpy(case["states"], case["k"], case["N"], case["logp"], case["branch_of"], log_thr=case["log_thr"])


@pytest.mark.parametrize("name", ALL_CASES)
def test_host_mirror_equals_numpy(name):
    case = get_case(name)
    host = run_host(case)
    same_db(host, run_numpy(case))
    well_formed(host)
    if name not in ("nothing",):
        assert host.num_entries > 0, "the case is vacuous"


def test_host_threads_give_the_same_bytes():
    case = get_case(CHUNKING_CASE)
    same_db(run_host(case, num_threads=1), run_host(case, num_threads=5))


def test_unpruned_and_frontier_restatements_agree(monkeypatch):
    case = get_case("nucl-k5-L63-G3")
    plain = run_numpy(case)
    monkeypatch.setattr(build, "UNPRUNED_CODES", 1)
    same_db(plain, run_numpy(case))


def test_threshold_seam():
    case = get_case("nucl-k5-L63-G3")
    base = run_host(case)
    lowest = base.values["score"].min()
    at = np.flatnonzero(base.values["score"] == lowest)
    case["log_thr"] = np.float32(lowest)  # the bits of that k-mer's sum: kept
    kept = run_host(case)
    same_db(kept, run_numpy(case))
    assert kept.values.tobytes() == base.values.tobytes() and np.array_equal(kept.keys, base.keys)
    case["log_thr"] = np.nextafter(np.float32(lowest), np.float32(0))  # one step above: dropped, nothing else changes
    dropped = run_host(case)
    same_db(dropped, run_numpy(case))
    assert dropped.num_entries == base.num_entries - len(at)
    assert dropped.values.tobytes() == np.delete(base.values, at).tobytes()


def test_everything_survives():
    case = get_case("everything")
    db = run_host(case)
    assert np.array_equal(db.keys, np.arange(4 ** 6, dtype=np.uint32)) and db.num_entries == 2 * 4 ** 6
    assert np.array_equal(db.values["branch"], np.tile(np.array([0, 2], dtype=np.uint32), 4 ** 6))


def test_nothing_survives():
    db = run_host(get_case("nothing"))
    assert db.keys.shape == (0,) and db.values.shape == (0,) and db.offsets.tolist() == [0]


def test_special_values():
    db = run_host(get_case("special"))
    assert np.all(np.isfinite(db.values["score"])), "a k-mer with p = 0 survived"
    zero = db.values["score"].view(np.uint32) == 0
    assert zero.any(), "no k-mer of probability 1 was carried through"
    same_db(db, run_host(get_case("special-negative-zero")))


def test_best_of_several():
    case = get_case("periodic")
    db = run_host(case)
    k = case["k"]
    key = 0
    for c in case["letters"][:k]:
        key = key * 4 + int(c)
    logp = case["logp"]

    def score(g, w):
        s = np.float32(0)
        for j in range(k):
            s = np.float32(s + logp[g, w + j, case["letters"][w + j]])
        return s

    assert np.array_equal(case["letters"][0:k], case["letters"][4:4 + k]) and np.array_equal(case["letters"][0:k], case["letters"][8:8 + k])
    i = int(np.searchsorted(db.keys, key))
    assert db.keys[i] == key
    mine = db.values[int(db.offsets[i]):int(db.offsets[i + 1])]
    assert mine["branch"].tolist() == [1, 3]
    on_one = [score(0, 0), score(0, 4), score(0, 8), score(1, 0), score(1, 4), score(1, 8)]
    assert len(set(float(s) for s in on_one)) > 2
    assert mine["score"][0] == max(on_one) and mine["score"][1] == max(score(2, 0), score(2, 4), score(2, 8))
    assert max(on_one) == score(0, 4)  # the middle stretch of ghost node 0, not the first window met


def test_rounding_order_matters():
    case = get_case("rounding")
    logp, k = case["logp"], case["k"]
    node = logp[0]
    best = node.max(axis=1)
    W = node.shape[0] - k + 1
    left = np.zeros(W, dtype=np.float32)
    for j in range(k):
        left = (left + best[j:j + W]).astype(np.float32)
    terms = [best[j:j + W] for j in range(k)]
    while len(terms) > 1:
        terms = [(terms[i] + terms[i + 1]).astype(np.float32) for i in range(0, len(terms), 2)]
    assert np.any(left.view(np.uint32) != terms[0].view(np.uint32)), "the two association orders agree: the case is vacuous"
    same_db(run_host(case), run_numpy(case))


def test_logp_from_posteriors():
    p = np.array([1.0, 0.5, 0.0, -0.25, 0.001], dtype=np.float32)
    got = build.logp_from_posteriors(p)
    assert got.dtype == np.float32 and got[0] == 0 and np.signbit(got[0]) == False and np.isneginf(got[2]) and np.isneginf(got[3])  # noqa: E712
    assert got[1] == alphabet.log_threshold(np.float32(0.5)) and got[4] == alphabet.log_threshold(np.float32(0.001))


def _refused(match, **kw):
    args = dict(states="nucl", kmer_size=4, num_branches=3, logp=np.full((2, 6, 4), -0.5, dtype=np.float32),
                branch_of=np.array([0, 2], dtype=np.uint32))
    args.update(kw)
    with pytest.raises(capi.EpikAmdError, match=match) as info:
        build.build_host(**args)
    assert info.value.code == capi.ERR_INVALID


def test_host_refusals():
    bad = np.full((2, 6, 4), -0.5, dtype=np.float32)
    bad[1, 4, 2] = np.nan
    bad[1, 5, 0] = 0.5
    _refused(r"ghost node 1, site 4, state 2: logp is NaN", logp=bad)
    bad[1, 4, 2] = -1.0
    _refused(r"ghost node 1, site 5, state 0: logp is above 0", logp=bad)
    _refused(r"branch_of\[1\] = 3 is no branch of a tree of 3", branch_of=np.array([0, 3], dtype=np.uint32))
    _refused(r"L = 6 sites hold no window of k = 7", kmer_size=7)
    _refused(r"k = 1 is outside \[2, 15\] for sigma = 4", kmer_size=1)
    _refused(r"k = 16 is outside \[2, 15\] for sigma = 4", kmer_size=16, logp=np.full((1, 20, 4), -0.5, dtype=np.float32),
             branch_of=np.array([0], dtype=np.uint32))
    _refused(r"k = 8 is outside \[2, 7\] for sigma = 20", states="amino", kmer_size=8, logp=np.full((1, 9, 20), -0.5, dtype=np.float32),
             branch_of=np.array([0], dtype=np.uint32))
    _refused(r"log_thr must be a number that is at most 0", log_thr=np.float32(0.1))
    _refused(r"log_thr must be a number that is at most 0", log_thr=np.float32(np.nan))
    lib = capi.load()
    import ctypes
    handle = ctypes.c_void_p()
    rc = lib.epik_amd_build_host(5, 4, 3, ctypes.c_float(-1.0), None, None, 0, 6, 1, ctypes.byref(handle))
    assert rc == capi.ERR_INVALID and b"sigma = 5 is neither 4 nor 20" in lib.epik_amd_last_error() and not handle.value


def test_builder_exports():
    lib = capi.load()
    for name in ("epik_amd_builder_create", "epik_amd_builder_add", "epik_amd_builder_add_device", "epik_amd_builder_finish",
                 "epik_amd_builder_copy", "epik_amd_builder_destroy", "epik_amd_build_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)


# ---- the file side: newick.py, epik.py extend, the posterior reader, epik.py build -----------------------------------

from click.testing import CliRunner  # noqa: E402

from epik_amd import dbbuild, dbfile, newick, synth  # noqa: E402

EPIK_PY = os.path.join(ROOT, "epik.py")


def load_epik_py():
    import importlib.util
    spec = importlib.util.spec_from_file_location("epik_launcher", EPIK_PY)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def reroot(tree, new_root, suppress_old_root=False):
    """The same unrooted tree written from another node (what a reconstruction tool may do to the tree it is given);
    suppress_old_root: the old root, left with two neighbours, is taken out and its two edges joined."""
    near = [[(c, tree.length[c]) for c in tree.children[i]] for i in range(tree.num_nodes)]
    for i, p in enumerate(tree.parent):
        if p >= 0:
            near[i].append((p, tree.length[i]))
    if suppress_old_root and len(near[tree.root]) == 2 and new_root != tree.root:
        (a, la), (b, lb) = near[tree.root]
        near[a] = [(x, l) if x != tree.root else (b, (la or 0) + (lb or 0)) for x, l in near[a]]
        near[b] = [(x, l) if x != tree.root else (a, (la or 0) + (lb or 0)) for x, l in near[b]]
        near[tree.root] = []
    out = newick.Tree()

    def emit(node, came_from, length):
        kids = [emit(x, node, l) for x, l in near[node] if x != came_from]
        out.parent.append(-1), out.children.append(kids), out.length.append(length), out.label.append(tree.label[node]), out.edge.append(None)
        for c in kids:
            out.parent[c] = out.num_nodes - 1
        return out.num_nodes - 1

    emit(new_root, -1, None)
    return out


def forged_build_input(n_leaves=40, sites=200, seed=21, reads_per_branch=50, read_length=60):
    """The end-to-end input of the issue: per branch a random sequence, ghost posteriors 0.97 on it and 0.01 elsewhere,
    and reads cut from it."""
    rng = np.random.default_rng(seed)
    tree = synth.make_tree(n_leaves, seed=seed)
    branches = tree.num_nodes - 1
    seqs = rng.integers(0, 4, size=(branches, sites))
    post = np.full((branches, sites, 4), 0.01, dtype=np.float32)
    np.put_along_axis(post, seqs[..., None], np.float32(0.97), axis=2)
    chars = np.frombuffer(b"ACGT", dtype=np.uint8)
    reads, source = [], []
    for b in range(branches):
        for at in rng.integers(0, sites - read_length + 1, size=reads_per_branch):
            reads.append(chars[seqs[b, at:at + read_length]].tobytes().decode())
            source.append(b)
    return tree, post, reads, np.array(source)


def write_ar_files(folder, tree, post, states="nucl", order=None, reroot_at=None, suppress=False, extra_nodes=True):
    """tree.nwk, the extended tree written back with labelled inner nodes, and the posterior table of its ghost nodes
    (both ghost nodes of a branch carry the branch's posteriors) with rows of other nodes between them."""
    folder = str(folder)
    ref = newick.parse(tree.newick())
    with open(os.path.join(folder, "tree.nwk"), "w") as fh:
        fh.write(tree.newick() + "\n")
    ext = dbbuild.extended_tree(ref, inner_labels=True)
    if reroot_at is not None:
        ext = reroot(ext, ext.label.index(reroot_at), suppress)
    with open(os.path.join(folder, "ar.tree"), "w") as fh:
        fh.write(newick.write(ext) + "\n")
    letters = alphabet.state_chars(states)
    order = list(order or letters)
    with open(os.path.join(folder, "ar.probs"), "w") as fh:
        fh.write("Node\tSite\tState\t" + "\t".join(f"p_{c}" for c in order) + "\n")
        for b in range(post.shape[0]):
            for label in (f"M{b}", f"P{b}"):
                for site in range(post.shape[1]):
                    row = [f"{post[b, site, letters.index(c)]:.5f}" for c in order]
                    fh.write(f"{label}\t{site + 1}\t{order[int(np.argmax(post[b, site]))]}\t" + "\t".join(row) + "\n")
            if extra_nodes and b % 3 == 0:
                for site in range(post.shape[1]):
                    fh.write(f"I{1000 + b}\t{site + 1}\tA\t" + "\t".join(["0.25000"] * len(order)) + "\n")
    return os.path.join(folder, "tree.nwk"), os.path.join(folder, "ar.probs"), os.path.join(folder, "ar.tree")


def test_newick_numbers_nodes_like_the_driver():
    for leaves, seed in ((1, 1), (2, 2), (3, 3), (40, 4), (257, 5)):
        tree = synth.make_tree(leaves, seed=seed)
        parsed = newick.parse(tree.newick(jplace=True))
        assert parsed.edge == list(range(tree.num_nodes)) and parsed.root == tree.num_nodes - 1
        assert parsed.parent == [int(p) for p in tree.parent]
        assert parsed.children == [[int(c) for c in kids if c >= 0] for kids in tree.children]
        assert parsed.label == list(tree.labels)
        assert np.array_equal(np.array(parsed.length), tree.branch_length)
        assert newick.parse(newick.write(parsed, edges=True)).edge[:-1] == list(range(tree.num_nodes - 1))
    quoted = newick.parse("((a:1,'b c''d':2)x:0.5[comment],\n(e,f,g)'y z':3)root;")
    assert quoted.label == ["a", "b c'd", "x", "e", "f", "g", "y z", "root"] and quoted.children[6] == [3, 4, 5]
    assert quoted.length[3] is None and quoted.length[2] == 0.5
    assert newick.parse(newick.write(quoted)).label == quoted.label
    for text, message in (("(a,b)", "no final ';'"), ("(a,b;", "before the tree is closed"), ("(a,b));", r"'\)' without"),
                          ("(a:x,b);", "is no branch length"), ("(a,b);c", "after the final"), ("(a,,b);", "where a node should be"),
                          ("(a,\n(b,'c);", r"line 2, character 4: a quoted label")):
        with pytest.raises(newick.NewickError, match=message):
            newick.parse(text)


def test_extend_writes_the_ghost_nodes(tmp_path):
    tree = synth.make_tree(6, seed=8)
    n = tree.num_nodes
    ref = newick.parse(tree.newick())
    rng = np.random.default_rng(3)
    leaves = [i for i in range(n) if tree.children[i, 0] < 0]
    rows = {tree.labels[i]: "".join(rng.choice(list("ACGT"), size=12)) for i in leaves}
    gappy = {name: seq[:3] + ("-" if j < 4 else seq[3]) + seq[4:7] + "-" + seq[8:] for j, (name, seq) in enumerate(rows.items())}
    (tmp_path / "tree.nwk").write_text(tree.newick() + "\n")
    (tmp_path / "ref.fasta").write_text("".join(f">{name} some words\n{seq[:7]}\n{seq[7:]}\n" for name, seq in gappy.items()))
    runner, launcher = CliRunner(), load_epik_py()
    out = tmp_path / "out"
    result = runner.invoke(launcher.epik, ["extend", "-t", str(tmp_path / "tree.nwk"), "-r", str(tmp_path / "ref.fasta"), "-o", str(out)])
    assert result.exit_code == 0, result.output
    ext = newick.parse((out / "extended.nwk").read_text())
    assert ext.num_nodes == n + 4 * (n - 1) and sorted(x for x in ext.label if x.startswith("ghost_")) == sorted(
        name for b in range(n - 1) for name in dbbuild.ghost_names(b))
    depth_sum, leaf_count = np.zeros(n), np.zeros(n)
    for i in range(n):
        if tree.children[i, 0] < 0:
            leaf_count[i] = 1
        else:
            for c in tree.children[i]:
                leaf_count[i] += leaf_count[c]
                depth_sum[i] += depth_sum[c] + leaf_count[c] * tree.branch_length[c]
    for b in range(n - 1):
        g1 = ext.label.index(f"ghost_{b}_1")
        p = ext.parent[g1]
        m = ext.parent[p]
        assert ext.children[p] == [g1, ext.label.index(f"ghost_{b}_2")] and ext.length[g1] == 0.01 == ext.length[g1 + 1]
        below = [c for c in ext.children[m] if c != p][0]
        assert ext.length[m] == pytest.approx(tree.branch_length[b] / 2, rel=1e-15) and ext.length[below] == ext.length[m]
        assert ext.length[p] == pytest.approx(tree.branch_length[b] / 2 + depth_sum[b] / leaf_count[b], rel=1e-12)
        if tree.children[b, 0] < 0:
            assert ext.label[below] == tree.labels[b] and ext.length[p] == pytest.approx(tree.branch_length[b] / 2, rel=1e-12)
    # written back without labels it is no use to `build`; with labels the ghost nodes are found
    with pytest.raises(dbbuild.BuildInputError, match="node of branch 0 has no label"):
        dbbuild.ghost_node_labels(ref, ext)
    records = dbbuild.read_fasta(str(out / "extended.fasta"))
    assert [r[0] for r in records[:len(gappy)]] == list(gappy) and [r[1] for r in records[:len(gappy)]] == list(gappy.values())
    assert [r[0] for r in records[len(gappy):]] == [name for b in range(n - 1) for name in dbbuild.ghost_names(b)]
    assert all(r[1] == "-" * 12 for r in records[len(gappy):])
    assert (out / "columns.tsv").read_text().splitlines() == ["column\toriginal"] + [f"{i}\t{i}" for i in range(12)]
    # the reduction: column 7 is all gaps, column 3 has 4 of 6
    for r, kept in ((1.0, [c for c in range(12) if c != 7]), (0.6, [c for c in range(12) if c not in (3, 7)]), (0.7, [c for c in range(12) if c != 7])):
        out_r = tmp_path / f"out_{r}"
        result = runner.invoke(launcher.epik, ["extend", "-t", str(tmp_path / "tree.nwk"), "-r", str(tmp_path / "ref.fasta"), "-o", str(out_r),
                                               "--reduction", str(r)])
        assert result.exit_code == 0, result.output
        assert (out_r / "columns.tsv").read_text().splitlines()[1:] == [f"{i}\t{c}" for i, c in enumerate(kept)]
        reduced = dbbuild.read_fasta(str(out_r / "extended.fasta"))
        assert reduced[0][1] == "".join(list(gappy.values())[0][c] for c in kept) and reduced[-1][1] == "-" * len(kept)


def test_extend_errors(tmp_path):
    runner, launcher = CliRunner(), load_epik_py()

    def refused(tree_text, fasta_text, message):
        (tmp_path / "t.nwk").write_text(tree_text)
        (tmp_path / "r.fasta").write_text(fasta_text)
        result = runner.invoke(launcher.epik, ["extend", "-t", str(tmp_path / "t.nwk"), "-r", str(tmp_path / "r.fasta"), "-o", str(tmp_path / "o")])
        assert result.exit_code == 2 and message in result.output.replace("\n", " "), result.output
        assert not (tmp_path / "o").exists()

    good = ">a\nACGT\n>b\nACGT\n>c\nAC-T\n"
    refused("((a:1,b:1):1,c:2);", ">a\nACGT\n>b\nACGT\n", "the leaf 'c' has no sequence")
    refused("((a:1,b:1):1,c:2);", ">a\nACGT\n>b\nACG\n>c\nACGT\n", "the sequence 'b' has 3 columns, 'a' has 4")
    refused("((a:1,b:1,d:1):1,c:2);", good + ">d\nACGT\n", "has 3 children")
    refused("((a:1,ghost_1_1:1):1,c:2);", good, "collides with the ghost nodes' names")
    refused("((a:1,b:1):1,c:2);", good + ">ghost_x\nACGT\n", "the name 'ghost_x' collides")
    refused("((a:1,b:1):1,c:2;", good, "before the tree is closed")
    refused("((a:1,b:1):1,c:2);", good + ">a\nACGT\n", "the sequence 'a' is given twice")


def small_posterior_case(tmp_path, **kw):
    tree = synth.make_tree(4, seed=2)
    rng = np.random.default_rng(1)
    post = np.round(rng.dirichlet(np.full(4, 0.3), size=(tree.num_nodes - 1, 9)), 5).astype(np.float32)
    return tree, post, write_ar_files(tmp_path, tree, post, **kw)


def test_posterior_reader_follows_the_header(tmp_path):
    plain_dir, mixed_dir = tmp_path / "plain", tmp_path / "mixed"
    plain_dir.mkdir(), mixed_dir.mkdir()
    tree, post, (_, plain, _) = small_posterior_case(plain_dir)
    _, _, (_, mixed, _) = small_posterior_case(mixed_dir, order="TGAC")
    wanted = {f"M{b}": b for b in range(post.shape[0])}
    got = {}
    for path in (plain, mixed):
        with open(path) as fh:
            got[path] = list(dbbuild.ghost_posteriors(fh, "nucl", wanted, path))
        assert [label for label, _ in got[path]] == [f"M{b}" for b in range(post.shape[0])]  # P and I nodes are skipped
        for b, (_, p) in enumerate(got[path]):
            assert p.dtype == np.float32 and np.array_equal(p, post[b])


def test_posterior_reader_errors_name_the_line(tmp_path):
    tree, post, (_, probs, _) = small_posterior_case(tmp_path)
    lines = open(probs).read().splitlines()
    wanted = {"M0": 0, "P0": 0, "M1": 1}

    def refused(edit, message, states="nucl"):
        changed = list(lines)
        edit(changed)
        path = tmp_path / "bad.probs"
        path.write_text("\n".join(changed) + "\n")
        with pytest.raises(dbbuild.BuildInputError, match=message):
            with open(path) as fh:
                list(dbbuild.ghost_posteriors(fh, states, wanted, "bad.probs"))

    def set_field(line, col, text):
        def edit(changed):
            fields = changed[line - 1].split("\t")
            fields[col] = text
            changed[line - 1] = "\t".join(fields)
        return edit

    assert lines[1].startswith("M0\t1\t") and lines[10].startswith("P0\t1\t")
    refused(lambda c: c.pop(4), r"bad.probs, line 9: node 'M0' \(from line 2\) ends with site 4 missing")
    refused(set_field(5, 1, "3"), r"bad.probs, line 5: site 3 of node 'M0' is given twice")
    refused(set_field(12, 4, "1.5"), r"bad.probs, line 12: the probability 1.5 lies outside \[0, 1\]")
    refused(set_field(12, 5, "-0.1"), r"bad.probs, line 12: the probability -0.1 lies outside")
    refused(set_field(12, 6, "nan"), r"bad.probs, line 12: the probability nan lies outside")
    refused(set_field(3, 3, "x.y"), r"bad.probs, line 3: 'x.y' is no number")
    refused(set_field(3, 1, "two"), r"bad.probs, line 3: 'two' is no site number")
    refused(set_field(3, 1, "0"), r"bad.probs, line 3: site 0 \(sites are 1-based\)")
    refused(lambda c: c.__setitem__(2, "M0\t2"), r"bad.probs, line 3: 2 fields, the header has more")
    refused(lambda c: c.pop(18), r"bad.probs, line 18: node 'P0' \(from line 11\) has 8 sites, the ghost nodes before it have 9")
    refused(lambda c: c.append(c[1]), r"line \d+: the rows of node 'M0' are not together")
    refused(set_field(1, 4, "p_X"), r"bad.probs, line 1: the header has no column 'p_C' for state C")
    refused(set_field(1, 0, "Name"), r"bad.probs, line 1: the header has no 'Node' column")
    refused(lambda c: None, r"line 1: the header has no column 'p_R' for state R", states="amino")


def test_ghost_nodes_are_found_however_the_tree_is_rooted(tmp_path):
    tree = synth.make_tree(9, seed=6)
    ref = newick.parse(tree.newick())
    ext = dbbuild.extended_tree(ref, inner_labels=True)
    want = [(f"M{b}", f"P{b}") for b in range(tree.num_nodes - 1)]
    assert dbbuild.ghost_node_labels(ref, newick.parse(newick.write(ext))) == want
    for at in ("P3", "M0", "I%d" % next(i for i in range(tree.num_nodes - 1) if tree.children[i, 0] >= 0), "M%d" % (tree.num_nodes - 2)):
        for suppress in (False, True):
            written = newick.parse(newick.write(reroot(ext, ext.label.index(at), suppress)))
            assert written.num_nodes == ext.num_nodes - (1 if suppress else 0)
            assert dbbuild.ghost_node_labels(ref, written) == want
    # what is wrong names the branch
    def broken(edit, message):
        text = edit(newick.write(ext))
        with pytest.raises(dbbuild.BuildInputError, match=message):
            dbbuild.ghost_node_labels(ref, newick.parse(text))
    broken(lambda s: s.replace("ghost_4_2", "ghost_4_3"), "no leaf 'ghost_4_2': branch 4 has no ghost nodes")
    broken(lambda s: s.replace(")P5:", "):"), "the pendant node of branch 5 has no label")
    broken(lambda s: s.replace(")M5:", "):"), "the midpoint node of branch 5 has no label")
    other = synth.make_tree(9, seed=7)
    with pytest.raises(dbbuild.BuildInputError, match=r"is not the extension of the reference tree at branch \d+"):
        dbbuild.ghost_node_labels(newick.parse(other.newick()), newick.parse(newick.write(ext)))


def test_build_refusals_before_anything_is_opened(tmp_path):
    runner, launcher = CliRunner(), load_epik_py()
    missing = [str(tmp_path / name) for name in ("no.nwk", "no.probs", "no.tree")]
    out = tmp_path / "db.ekdb"

    def refused(arguments, message, files=missing):
        result = runner.invoke(launcher.epik, ["build", "-t", files[0], "--ar-probs", files[1], "--ar-tree", files[2], "-o", str(out)] + arguments)
        assert result.exit_code == 2 and message in result.output.replace("\n", " "), result.output
        assert not out.exists()

    # (the files do not exist: an option that is refused is refused before they are looked for)
    refused(["-k", "16"], "-k must lie in [2, 15] for -s nucl, not 16")
    refused(["-k", "1"], "-k must lie in [2, 15] for -s nucl, not 1")
    refused(["-k", "8", "-s", "amino"], "-k must lie in [2, 7] for -s amino, not 8")
    refused(["-k", "8", "--omega", "0"], "--omega must lie in (0, 4]")
    refused(["-k", "8", "--omega", "4.5"], "--omega must lie in (0, 4]")
    refused(["-k", "8", "--chunk", "0"], "--chunk must be at least 1")
    refused(["-k", "8", "--ghosts", "all"], "'all' is not one of")
    refused(["-k", "8"], "-t: the file")
    refused([], "Missing option '-k'")
    launcher_commands = sorted(launcher.epik.commands)
    assert launcher_commands == ["build", "extend", "place"]


@pytest.fixture(scope="module")
def forged():
    return forged_build_input()


def test_forged_reads_go_home_on_the_cpu(forged, oracle_lib):
    """The end-to-end claim of test_dbbuild_gpu.py, checked here first with the host mirror and the CPU oracle: every
    read's best row is on the branch it was cut from."""
    tree, post, reads, source = forged
    logp = build.logp_from_posteriors(np.concatenate([post, post]))
    branch_of = np.concatenate([np.arange(post.shape[0]), np.arange(post.shape[0])]).astype(np.uint32)
    db = build.build_host("nucl", 8, tree.num_nodes, logp, branch_of, omega=1.5, num_threads=4)
    well_formed(db)
    data, offs = synth.pack_reads(reads)
    rows, n_rows, _ = oracle_lib.Oracle.from_synth(db).place(data, offs, num_threads=0)
    assert np.all(n_rows >= 1) and np.array_equal(rows[:, 0]["branch"], source)


def test_build_from_files_equals_the_build_in_memory(tmp_path, forged):
    """The file side without a device: the posterior table written out and streamed back in chunks gives the database
    of the arrays it was written from, and dbfile reads it back."""
    tree, post, _, _ = forged
    post = post[:, :40]
    tree_path, probs, ar_tree = write_ar_files(tmp_path, tree, post, reroot_at="P7", suppress=True)
    out = str(tmp_path / "db.ekdb")
    for ghosts, copies in (("both", 2), ("inner", 1)):
        info = dbbuild.build_from_files(tree_path, probs, ar_tree, "nucl", 6, 1.5, out, ghosts=ghosts, chunk=7, host=True)
        branch_of = np.tile(np.arange(post.shape[0]), copies).astype(np.uint32)
        want = build.build_host("nucl", 6, tree.num_nodes, build.logp_from_posteriors(np.concatenate([post] * copies)), branch_of)
        assert info["ghost_nodes"] == copies * post.shape[0] and info["num_entries"] == want.num_entries
        got, text = dbfile.read_db(out)
        dense = want.densified()
        assert text == tree.newick() and got.num_branches == tree.num_nodes and got.kmer_size == 6
        assert np.array_equal(got.offsets, dense.offsets) and got.values.tobytes() == dense.values.tobytes()
    with pytest.raises(dbbuild.BuildInputError, match="no rows for node 'M3', a ghost node of branch 3"):
        lines = [line for line in open(probs) if not line.startswith("M3\t")]
        (tmp_path / "short.probs").write_text("".join(lines))
        dbbuild.build_from_files(tree_path, str(tmp_path / "short.probs"), ar_tree, "nucl", 6, 1.5, out, host=True)
