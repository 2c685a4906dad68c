"""Placement confidence without a GPU (include/epik_amd.h: epik_amd_tree, epik_amd_confidence): the rule written out
here over walks up parent[] -- it shares nothing with the library but the header's text --, the hand values of the
rule, the LCA tables of libepik_amd (the function the kernel calls, on the host) against that walk, every validation
error by the branch it names, the host mirror (epik_amd/host/confidence.cpp, through bin/confidence_test) against the
restatement bit for bit on oracle rows and on forged rows (forged_batch: every class and every edge of the rule's
arithmetic, at eight values of keep on six trees), both TSVs both ways, the flags of the launcher and the drivers, the
new symbols."""
import ctypes
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

try:  # torch first: its HIP runtime must be the process's before libepik_amd's loads (capi.check_hip_runtime)
    import torch  # noqa: F401
except ImportError:
    pass

from conftest import mixed_reads
from epik_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")
LWR_BITS = 30
TOO_NARROW = 0xFFFFFFFF
M64 = (1 << 64) - 1
CLADE_TOO_NARROW, CLADE_TOO_SHORT, CLADE_NO_HIT, CLADE_BAD_ROW = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
HAND_NEWICK = "((A:1,B:2)C:3,(D:4,E:5)F:6)R:0"
HAND_PARENT = [2, 2, 6, 5, 5, 6, -1]
HAND_LENGTH = [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 0.0]


def q(x):
    """llrint(x * 2^30), round half to even."""
    return int(np.rint(np.float64(x) * np.float64(1 << LWR_BITS)))


class RuleTree:
    """The tree of the rule from parent[] (-1: the root) and the branch lengths: size, first, depth, mid; lca by a walk
    up parent[] -- the chain of ancestors of a node, kept once it has been walked."""

    def __init__(self, parent, branch_length):
        self.parent = [int(x) for x in parent]
        self.n = n = len(self.parent)
        self.length = [float(x) for x in branch_length]
        self.size = [1] * n
        for b in range(n - 1):
            self.size[self.parent[b]] += self.size[b]
        self.first = [b - self.size[b] + 1 for b in range(n)]
        self.depth = [0.0] * n
        for b in range(n - 1, -1, -1):
            self.depth[b] = (self.depth[self.parent[b]] if b < n - 1 else 0.0) + self.length[b]
        self.mid = [self.depth[b] - self.length[b] / 2 for b in range(n)]
        self._known = {}

    def lca(self, a, b):
        """A walk up parent[] from the higher id until the node's clade holds both (kept once walked)."""
        key = (a, b) if a < b else (b, a)
        if key not in self._known:
            lo, c = min(self.first[a], self.first[b]), max(a, b)
            while self.first[c] > lo:
                c = self.parent[c]
            self._known[key] = c
        return self._known[key]

    def walk_many(self, a, b):
        """The same walk for many pairs at once: every pair steps up until its node's clade holds both."""
        a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
        parent, first = np.array(self.parent, dtype=np.int64), np.array(self.first, dtype=np.int64)
        lo, c = np.minimum(first[a], first[b]), np.maximum(a, b)
        while True:
            up = first[c] > lo
            if not up.any():
                return c
            c[up] = parent[c[up]]

    def learn(self, a, b):
        """Walks many pairs at once and keeps the answers for lca()."""
        for x, y, c in zip(a, b, self.walk_many(a, b)):
            self._known[(int(x), int(y)) if x < y else (int(y), int(x))] = int(c)

    def inside(self, x, b):
        return self.first[b] <= x <= b

    def distance(self, a, b):
        if a == b:
            return 0.0
        if self.inside(a, b):
            return self.mid[a] - self.mid[b]
        if self.inside(b, a):
            return self.mid[b] - self.mid[a]
        c = self.lca(a, b)
        return (self.mid[a] - self.depth[c]) + (self.mid[b] - self.depth[c])


def rule_record(tree, branches, lwrs, n_rows, first_count, keep, tau_q):
    """The record of one read: (clade, clade_mass_q, edpl)."""
    if n_rows == TOO_NARROW:
        return CLADE_TOO_NARROW, 0, 0.0
    if n_rows == 0:
        return CLADE_TOO_SHORT, 0, 0.0
    if first_count == 0:
        return CLADE_NO_HIT, 0, 0.0
    nr = min(int(n_rows), keep)
    b = [int(x) for x in branches[:nr]]
    if any(x >= tree.n for x in b):
        return CLADE_BAD_ROW, 0, 0.0
    w = [float(x) for x in lwrs[:nr]]
    qs = [q(x) for x in w]
    total, prefix, m = sum(qs) & M64, 0, nr
    for k in range(nr):
        prefix = (prefix + qs[k]) & M64
        if ((prefix << LWR_BITS) & M64) >= ((tau_q * total) & M64):
            m = k + 1
            break
    clade = b[0]
    for x in b[1:m]:
        clade = tree.lca(clade, x)
    mass = min(sum(qs[k] for k in range(nr) if tree.inside(b[k], clade)), 0xFFFFFFFF)
    total_d = 0.0
    for j in range(nr):
        for l in range(j + 1, nr):
            total_d = total_d + (w[j] * w[l]) * tree.distance(b[j], b[l])
    return clade, mass, 2.0 * total_d


def numpy_rule(tree, rows, n_rows, counts, tau_q):
    """The records of a batch as capi.CONFIDENCE; slots past n_rows are never looked at."""
    n, keep = rows.shape
    out = np.zeros(n, dtype=capi.CONFIDENCE)
    # (long walks -- a ladder-shaped tree -- are taken for all pairs of the batch at once; the rule below is read by read)
    live = np.where(n_rows == TOO_NARROW, 0, np.minimum(n_rows, keep)).astype(np.int64)
    ok = (np.arange(keep)[None, :] < live[:, None]) & (rows["branch"] < tree.n)
    pairs = ok[:, :, None] & ok[:, None, :] & (np.arange(keep)[:, None] < np.arange(keep)[None, :])[None]
    i_, j_, l_ = np.nonzero(pairs)
    if len(i_):
        both = np.unique(np.stack([rows["branch"][i_, j_], rows["branch"][i_, l_]], axis=1).astype(np.int64), axis=0)
        tree.learn(both[:, 0], both[:, 1])
    for i in range(n):
        nr = int(n_rows[i])
        live = 0 if nr == TOO_NARROW else min(nr, keep)
        out[i] = rule_record(tree, rows["branch"][i, :live], rows["lwr"][i, :live], nr, int(counts[i, 0]), keep, tau_q)
    return out


def same_bits(a, b):
    """Two arrays of records agree bit for bit, edpl included."""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def caterpillar(n_nodes, seed=3):
    """A ladder: every inner node has one leaf and the rest of the ladder below it.  n_nodes odd; (parent, lengths)."""
    assert n_nodes % 2 == 1
    parent = np.full(n_nodes, -1, dtype=np.int64)
    # post-order: leaf 0, leaf 1, inner 2 = (0, 1), leaf 3, inner 4 = (2, 3), ...
    parent[0] = parent[1] = 2
    for inner in range(2, n_nodes - 2, 2):
        parent[inner] = parent[inner + 1] = inner + 2
    lengths = np.random.default_rng(seed).uniform(0.01, 0.3, size=n_nodes)
    return parent, lengths


def poison(rows, n_rows, counts):
    """Garbage in every slot past n_rows: the rule must not look there."""
    rows, counts = rows.copy(), counts.copy()
    keep = rows.shape[1]
    live = np.where(n_rows == TOO_NARROW, 0, np.minimum(n_rows, keep)).astype(np.int64)
    dead = np.arange(keep)[None, :] >= live[:, None]
    rows["branch"][dead] = 0xFFFFFFFF
    rows["lwr"][dead] = np.nan
    rows["score"][dead] = np.nan
    counts[dead] = 0xFFFFFFFF
    return rows, counts


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


def write_tree(path, parent, lengths):
    from epik_amd.confidence import parents_of
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(parent)))
        fh.write(np.ascontiguousarray(parents_of(parent)).tobytes())
        fh.write(np.ascontiguousarray(lengths, dtype=np.float64).tobytes())


def write_input(path, rows, n_rows, counts, weights, parent, lengths):
    from epik_amd.confidence import parents_of
    n, keep = rows.shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("<3Q", n, keep, len(parent)))
        fh.write(np.ascontiguousarray(rows, dtype=capi.PLACEMENT).tobytes())
        fh.write(np.ascontiguousarray(n_rows, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(counts, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(weights, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(parents_of(parent)).tobytes())
        fh.write(np.ascontiguousarray(lengths, dtype=np.float64).tobytes())


def host_records(host_bins, tmp_path, rows, n_rows, counts, parent, lengths, tau_q):
    write_input(tmp_path / "in.bin", rows, n_rows, counts, np.ones(len(n_rows), np.uint32), parent, lengths)
    run = subprocess.run([os.path.join(host_bins, "confidence_test"), "records", str(tau_q), str(tmp_path / "in.bin"),
                          str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    return np.fromfile(tmp_path / "out.bin", dtype=capi.CONFIDENCE)


def hand_read(keep=7):
    rows = np.zeros((1, keep), dtype=capi.PLACEMENT)
    rows["branch"][0, :3], rows["lwr"][0, :3] = [0, 1, 3], [0.5, 0.25, 0.25]
    return rows, np.array([3], np.uint32), np.ones((1, keep), np.uint32)


def star(leaves, seed=5):
    """A star: every leaf hangs off the root, one multifurcation of `leaves` children.  (parent, lengths)."""
    parent = np.full(leaves + 1, leaves, dtype=np.int64)
    parent[leaves] = -1
    return parent, np.random.default_rng(seed).uniform(0.01, 0.3, size=leaves + 1)


def forged_batch(rng, n, keep, num_branches):
    """(rows, n_rows, counts) that no placement writes: every class of the rule and the edges of its arithmetic, by
    strides that cross each other (read i: LWRs by i % 8, n_rows by i // 8 % 8, the rest by 5, 11, 13 and 17).
      branches  uniform over [0, N); every fifth read draws from min(N, 3) branches only: repeats, adjacent rows included
      LWRs      finite, in [0, 1] a row: a sorted Dirichlet draw | all 1 / keep | all 0.0 (S == 0) | all 1.0 (clade_mass_q
                saturates from 5 rows up, S << 30 wraps from 16) | dyadics 2^-e in no order (prefix sums meet tau_q * S
                exactly) | 0.5, 0.25, 0.25 then zeros (hand_read; keep >= 3) | uniform, unsorted | a Dirichlet draw, unsorted
      n_rows    1 ... keep (three eighths) | keep (two) | keep + 5, which the rule clamps | 0 | TOO_NARROW
      counts    counts[i, 0] == 0 for every eleventh read
      bad rows  every thirteenth read has one row, anywhere below keep, of branch N, N + 1 or 0xFFFFFFFF: past the
                read's n_rows (not looked at), inside it but past the prefix, or inside the prefix
      clamped   every seventeenth read (N >= 3) has n_rows = keep + 5, every LWR 1.0 and a hit, and all its rows on one
                branch b, or on b and b + 1, with 1 <= b < N - 1: where S_m << 30 wraps past every threshold its prefix is
                all of its rows -- keep of them; a prefix of n_rows rows would run on into rows that are not the read's
    and poison() over every slot past n_rows."""
    N, i = int(num_branches), np.arange(n)
    rows = np.zeros((n, keep), dtype=capi.PLACEMENT)
    rows["branch"] = rng.integers(0, N, size=(n, keep))
    few = i % 5 == 2
    rows["branch"][few] = rng.integers(0, min(N, 3), size=(int(few.sum()), keep))
    rows["score"] = -rng.random((n, keep))
    kind = i % 8
    lwr = -np.sort(-rng.dirichlet(np.ones(keep), size=n), axis=1)
    lwr[kind == 1] = 1.0 / keep
    lwr[kind == 2] = 0.0
    lwr[kind == 3] = 1.0
    lwr[kind == 4] = 2.0 ** -rng.integers(0, 5, size=(int((kind == 4).sum()), keep)).astype(np.float64)
    if keep >= 3:
        lwr[kind == 5] = 0.0
        lwr[kind == 5, :3] = [0.5, 0.25, 0.25]
    lwr[kind == 6] = rng.random((int((kind == 6).sum()), keep))
    lwr[kind == 7] = rng.dirichlet(np.ones(keep), size=int((kind == 7).sum()))
    rows["lwr"] = lwr
    n_kind = i // 8 % 8
    n_rows = rng.integers(1, keep + 1, size=n).astype(np.uint32)
    n_rows[(n_kind == 3) | (n_kind == 4)] = keep
    n_rows[n_kind == 5] = keep + 5
    n_rows[n_kind == 6] = 0
    n_rows[n_kind == 7] = TOO_NARROW
    counts = rng.integers(1, 300, size=(n, keep)).astype(np.uint32)
    counts[i % 11 == 5, 0] = 0
    bad = np.nonzero(i % 13 == 3)[0]
    rows["branch"][bad, rng.integers(0, keep, size=len(bad))] = rng.choice([N, N + 1, 0xFFFFFFFF], size=len(bad))
    if N >= 3:
        over = np.nonzero(i % 17 == 7)[0]
        b = rng.integers(1, N - 1, size=len(over))
        pair = (np.arange(len(over)) % 2 == 1) & (b + 1 < N - 1)
        rows["branch"][over] = b[:, None] + (pair[:, None] & (rng.random((len(over), keep)) < 0.5))
        rows["lwr"][over], n_rows[over], counts[over, 0] = 1.0, keep + 5, 1
    rows, counts = poison(rows, n_rows, counts)
    return rows, n_rows, counts


def test_hand_values_in_numpy():
    from epik_amd.confidence import tau_q
    t = RuleTree(HAND_PARENT, HAND_LENGTH)
    assert t.depth == [4, 5, 3, 10, 11, 6, 0] and t.mid == [3.5, 4, 1.5, 8, 8.5, 3, 0]
    assert t.first == [0, 1, 0, 3, 4, 3, 0]
    assert (t.distance(0, 1), t.distance(0, 2), t.distance(0, 3), t.distance(1, 3)) == (1.5, 2, 11.5, 12)
    assert t.distance(2, 0) == 2 and t.distance(4, 4) == 0 and t.lca(0, 1) == 2 and t.lca(1, 3) == 6 and t.lca(0, 2) == 2
    rows, n_rows, counts = hand_read()
    for tau, clade, mass in ((0.5, 0, 1 << 29), (0.75, 2, 3 << 28), (0.95, 6, 1 << 30)):
        got = numpy_rule(t, rows, n_rows, counts, tau_q(tau))[0]
        assert (int(got["clade"]), int(got["clade_mass_q"]), float(got["edpl"])) == (clade, mass, 4.75), tau
    assert (tau_q(0), tau_q(0.5), tau_q(0.95), tau_q(1)) == (0, 1 << 29, int(np.rint(0.95 * 2 ** 30)), 1 << 30)
    with pytest.raises(ValueError):
        tau_q(1.5)


def test_hand_values_through_the_host_mirror(host_bins, tmp_path):
    from epik_amd.confidence import tau_q
    run = subprocess.run([os.path.join(host_bins, "confidence_test"), "tree", HAND_NEWICK + ";"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    table = [line.split() for line in run.stdout.split("\n") if line]
    assert [int(r[1]) for r in table] == HAND_PARENT and [int(r[2]) for r in table] == [0, 1, 0, 3, 4, 3, 0]
    assert [float(r[3]) for r in table] == [4, 5, 3, 10, 11, 6, 0] and [float(r[4]) for r in table] == [3.5, 4, 1.5, 8, 8.5, 3, 0]
    rows, n_rows, counts = hand_read()
    for tau, clade, mass in ((0.5, 0, 1 << 29), (0.75, 2, 3 << 28), (0.95, 6, 1 << 30)):
        got = host_records(host_bins, tmp_path, rows, n_rows, counts, HAND_PARENT, HAND_LENGTH, tau_q(tau))[0]
        assert (int(got["clade"]), int(got["clade_mass_q"]), float(got["edpl"])) == (clade, mass, 4.75), tau
    # one row: +0.0, the clade is the branch whatever tau
    rows["branch"][0, 0], n_rows[0] = 4, 1
    got = host_records(host_bins, tmp_path, rows, n_rows, counts, HAND_PARENT, HAND_LENGTH, 1 << 30)
    assert int(got["clade"][0]) == 4 and got["edpl"].view(np.uint64)[0] == 0 and int(got["clade_mass_q"][0]) == 1 << 29


MULTI_PARENT = [4, 4, 4, 4, 9, 8, 8, 8, 9, 11, 11, -1]    # ((a,b,c,d)e,(f,g,h)i)j,k)l: two multifurcations


def _trees():
    out = {}
    for leaves in (8, 1500, 5200):
        t = synth.make_tree(leaves, seed=30 if leaves > 8 else 1)
        out[f"synth{leaves}"] = (t.parent, t.branch_length)
    out["caterpillar10399"] = caterpillar(10399)
    out["multifurcating"] = (np.array(MULTI_PARENT), np.arange(12) * 0.5)
    out["one_branch"] = (np.array([-1]), np.array([0.25]))
    return out


@pytest.mark.parametrize("name", ["synth8", "synth1500", "synth5200", "caterpillar10399", "multifurcating", "one_branch"])
def test_lca_tables_against_a_parent_walk(name):
    from epik_amd.confidence import HostTables
    parent, lengths = _trees()[name]
    n = len(parent)
    tables = HostTables(parent, lengths)
    levels = max(1, int(np.ceil(np.log2(n)))) if n > 1 else 1
    assert tables.table_bytes == 32 + n * (16 + 8 * levels) + (4 * n + 7) // 8 * 8
    rule = RuleTree(parent, lengths)
    if n <= 16:
        a, b = [x.reshape(-1) for x in np.meshgrid(np.arange(n), np.arange(n))]
    else:
        rng = np.random.default_rng(n)
        a, b = rng.integers(0, n, size=100_000), rng.integers(0, n, size=100_000)
        a[:1000] = np.minimum(a[:1000] + 1, n - 1)                       # (neighbours, nested pairs, the same branch)
        b[:1000] = a[:1000] - 1
        b[1000:2000] = a[1000:2000]
        a[2000:3000] = np.array(rule.parent)[b[2000:3000]].clip(0)
    want = rule.walk_many(a, b)
    got = tables.lca(a, b)
    assert np.array_equal(got.astype(np.int64), want), np.nonzero(got != want)[0][:10]
    assert np.array_equal(tables.lca(b, a), got)
    if name == "multifurcating":
        assert rule.lca(0, 3) == 4 and rule.lca(2, 6) == 9 and rule.lca(5, 10) == 11 and rule.size[4] == 5
    # the single-pair walk of the restatement agrees with the one over arrays
    assert all(rule.lca(int(x), int(y)) == int(z) for x, y, z in zip(a[:200], b[:200], want[:200]))
    # a query outside the tree is refused
    lib, out = capi.load(), np.zeros(1, np.uint32)
    bad = np.array([n], np.uint32)
    assert lib.epik_amd_tree_lca_host(tables.tables.ctypes.data, bad.ctypes.data, bad.ctypes.data, 1, out.ctypes.data) == capi.ERR_INVALID


INVALID_TREES = [
    # (parent, lengths, the branch the error names)
    ([0, 2, 6, 5, 5, 6, -1], None, 0),                      # a parent not above its child: itself
    ([2, 2, 6, 2, 5, 6, -1], None, 3),                      # ... below it
    ([2, 7, 6, 5, 5, 6, -1], None, 1),                      # ... outside the tree
    ([2, 2, -1, 5, 5, 6, -1], None, 2),                     # a second root
    ([2, 2, 6, 5, 5, 6, 3], None, 6),                       # the last branch with a parent
    ([2, 3, 3, -1], [1.0] * 4, 2),                          # descendants of 2 are {0}, not [1, 2]
    ([3, 2, 4, 4, -1], [1.0] * 5, 3),                       # descendants of 3 are {0}, not [2, 3]
    (HAND_PARENT, [1, 2, 3, 4, -5.0, 6, 0], 4),             # a negative length
    (HAND_PARENT, [1, float("nan"), 3, 4, 5, 6, 0], 1),     # ... not a number
    (HAND_PARENT, [1, 2, 3, 4, 5, float("inf"), 0], 5),     # ... infinite
    ([0, 2, 6, 5, 5, 6, -1], [1, -2.0, 3, 4, 5, 6, 0], 0),  # two errors: the lower branch is named
]


@pytest.mark.parametrize("parent,lengths,branch", INVALID_TREES)
def test_every_validation_error_names_its_branch(host_bins, tmp_path, parent, lengths, branch):
    from epik_amd.confidence import HostTables, parents_of
    lengths = HAND_LENGTH if lengths is None else lengths
    with pytest.raises(capi.EpikAmdError) as e:
        HostTables(parent, lengths)
    assert e.value.code == capi.ERR_INVALID and f"branch {branch}:" in str(e.value), str(e.value)
    # create() validates before it looks for a device: the same refusal, with or without one
    lib, out = capi.load(), ctypes.c_void_p(7)
    p, bl = np.ascontiguousarray(parents_of(parent)), np.ascontiguousarray(lengths, dtype=np.float64)
    assert lib.epik_amd_tree_create(0, p.ctypes.data, bl.ctypes.data, len(parent), ctypes.byref(out)) == capi.ERR_INVALID
    assert not out.value and f"branch {branch}:".encode() in lib.epik_amd_last_error()
    write_tree(tmp_path / "tree.bin", parent, lengths)
    run = subprocess.run([os.path.join(host_bins, "confidence_test"), "validate", str(tmp_path / "tree.bin")], capture_output=True, text=True)
    assert run.returncode == 1 and run.stdout.startswith(f"branch {branch}:"), run.stdout + run.stderr


def test_valid_odd_trees_are_accepted(host_bins, tmp_path):
    from epik_amd.confidence import HostTables
    for parent, lengths in (_trees()["multifurcating"], _trees()["one_branch"], ([4, 2, 4, 4, -1], [0.0] * 5)):
        HostTables(parent, lengths)
        write_tree(tmp_path / "tree.bin", parent, lengths)
        run = subprocess.run([os.path.join(host_bins, "confidence_test"), "validate", str(tmp_path / "tree.bin")], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def _reads(k):
    return mixed_reads(np.random.default_rng(3), 600, k, alphabet_amb="ACGTNRYKMSWBDHV-", max_len=200) + ["ACG", "", "NNNNNNNNNN", "-" * 12]


@pytest.fixture(scope="module", params=["small", "large"])
def oracle_case(request, small_case):
    if request.param == "small":
        return small_case
    tree = synth.make_tree(1500, seed=30)
    return tree, synth.make_db(tree.num_nodes, kmer_size=4, seed=31, p_present=0.7)


@pytest.mark.parametrize("keep", [1, 7, 13])
def test_host_mirror_equals_the_rule_bit_for_bit_on_oracle_rows(host_bins, oracle_lib, oracle_case, tmp_path, keep):
    from epik_amd.confidence import tau_q
    tree, db = oracle_case
    rows, n_rows, counts = oracle_lib.Oracle.from_synth(db, keep_at_most=keep).place(*synth.pack_reads(_reads(db.kmer_size)), num_threads=0)
    rows = np.ascontiguousarray(rows).view(capi.PLACEMENT).reshape(rows.shape) if rows.dtype != capi.PLACEMENT else rows
    placed = (n_rows != 0) & (counts[:, 0] != 0)
    assert (n_rows == 0).sum() >= 2 and ((n_rows != 0) & (counts[:, 0] == 0)).sum() > 0 and placed.sum() > 500
    # a forged bad row and a forged TOO_NARROW read, then garbage in every slot the rule must not look at
    n_rows, rows = n_rows.copy(), rows.copy()
    victims = np.nonzero(placed)[0]
    rows["branch"][victims[0], int(n_rows[victims[0]]) - 1] = db.num_branches
    n_rows[victims[1]] = TOO_NARROW
    rows, counts = poison(rows, n_rows, counts)
    rule = RuleTree(tree.parent, tree.branch_length)
    for tau in (0, 0.5, 0.95, 1):
        want = numpy_rule(rule, rows, n_rows, counts, tau_q(tau))
        got = host_records(host_bins, tmp_path, rows, n_rows, counts, tree.parent, tree.branch_length, tau_q(tau))
        assert same_bits(got, want), (tau, np.nonzero(got != want)[0][:10])
        assert want["clade"][victims[0]] == CLADE_BAD_ROW and want["clade"][victims[1]] == CLADE_TOO_NARROW
        assert (want["clade"] == CLADE_TOO_SHORT).sum() == (n_rows == 0).sum() and (want["clade"] == CLADE_NO_HIT).sum() > 0
        ok = want["clade"] < db.num_branches
        assert ok.sum() == placed.sum() - 2 and not want["edpl"][~ok].any() and not want["clade_mass_q"][~ok].any()
        if tau == 0:
            assert np.array_equal(want["clade"][ok], rows["branch"][ok, 0])
        if tau == 0.95 and keep == 7:
            # not vacuous: most placed reads have several rows, and their clade is not simply their best branch
            several = (n_rows[ok] >= 2).sum()
            moved = (want["clade"][ok] != rows["branch"][ok, 0]).sum()
            print(f"N={db.num_branches}: {ok.sum()} placed reads, {several} with >= 2 rows, {moved} with a clade other than the best branch")
            assert 2 * several >= ok.sum() and 4 * moved >= ok.sum()
            assert (want["edpl"][ok][n_rows[ok] >= 2] > 0).all()
        if keep == 1:
            assert not want["edpl"].any() and np.array_equal(want["clade"][ok], rows["branch"][ok, 0])


FORGED_KEEPS = (1, 2, 3, 7, 8, 13, 33, 64)
FORGED_TAUS = (0, 1 << 29, int(np.rint(0.95 * 2 ** 30)), 1 << 30)      # 0, a half, tau_q(0.95), everything
FORGED_TREES = {}


def forged_tree(name):
    """(parent, lengths, RuleTree) of the trees the forged batches lie on; `ladder<nodes>` is a caterpillar of that many
    branches.  Some lengths are 0 (the hand tree keeps its own: its distances are written out above)."""
    if name not in FORGED_TREES:
        if name == "one_branch":
            parent, lengths = [-1], [0.25]
        elif name == "hand":
            parent, lengths = HAND_PARENT, HAND_LENGTH
        elif name == "multifurcating":
            parent, lengths = MULTI_PARENT, np.arange(12) * 0.5
        elif name == "star300":
            parent, lengths = star(300)
        elif name == "synth500":
            tree = synth.make_tree(500, seed=13)
            parent, lengths = tree.parent, tree.branch_length
        else:
            assert name.startswith("ladder"), name
            parent, lengths = caterpillar(int(name[len("ladder"):]))
        parent, lengths = np.array(parent, dtype=np.int64), np.array(lengths, dtype=np.float64)
        if len(parent) > 12:
            lengths[3::5] = 0.0
        FORGED_TREES[name] = (parent, lengths, RuleTree(parent, lengths))
    return FORGED_TREES[name]


def never_reached(qs, tq):
    """No prefix of the quantised LWRs qs meets tau_q * S in uint64: the rule's prefix is then all of the rows."""
    total = sum(qs)
    return all(((sum(qs[:m]) << LWR_BITS) & M64) < ((tq * total) & M64) for m in range(1, len(qs) + 1))


def assert_every_case_occurs(rule, rows, n_rows, counts, tq, want):
    """Conditions on a forged batch and on the records the restatement gives for it at tau_q = tq, none on the code under
    test: every class of the rule occurs, and every edge forged_batch is there to reach."""
    n, keep = rows.shape
    live = np.where(n_rows == TOO_NARROW, 0, np.minimum(n_rows, keep)).astype(np.int64)
    placed = want["clade"] < rule.n
    classes = {c: int((want["clade"] == c).sum()) for c in (CLADE_TOO_NARROW, CLADE_TOO_SHORT, CLADE_NO_HIT, CLADE_BAD_ROW)}
    assert placed.sum() > n // 4 and min(classes.values()) > 0, (tq, int(placed.sum()), classes)
    assert placed.sum() + sum(classes.values()) == n
    assert not want["edpl"][~placed].view(np.uint64).any() and not want["clade_mass_q"][~placed].any()
    saturated = int((want["clade_mass_q"][placed] == 0xFFFFFFFF).sum())
    moved = int((want["clade"][placed] != rows["branch"][placed, 0]).sum())
    # (the all-ones reads whose rows lie on one branch: five rows of them or more lie in their clade whatever tau_q)
    if keep >= 7:
        assert saturated > 0, tq
    # the clade is the first row's branch at tau_q 0.  Above it, a read moves off that branch when its first row holds
    # less than tau_q of S and a later row of the prefix lies outside the first one's clade.  Fewest do at keep 2 and a
    # half: the unsorted kinds (three eighths of the reads) where both rows are live (nine sixteenths) and the second is
    # the heavier (a half), a tenth of the reads less those whose two branches share a clade -- a thirty-second is well
    # below that.  With the whole mass it is every read of two rows or more that are not all in the clade of the first
    if tq == 0:
        assert moved == 0
    elif keep > 1 and rule.n > 1:
        assert moved >= placed.sum() // (8 if tq == 1 << 30 else 32), (moved, int(placed.sum()))
    ids = np.nonzero(placed)[0]
    q_of = {int(i): [q(x) for x in rows["lwr"][i, :live[i]]] for i in ids}
    branches = {int(i): [int(b) for b in rows["branch"][i, :live[i]]] for i in ids}
    assert ((n_rows[ids] > keep) & (n_rows[ids] != TOO_NARROW)).sum() > 0      # n_rows beyond keep: clamped
    assert sum(1 for i in q_of if not any(q_of[i])) > 0                        # S == 0
    if keep > 1:
        assert sum(1 for b in branches.values() if len(set(b)) < len(b)) > 0                        # a branch twice in a read
        assert sum(1 for b in branches.values() if any(x == y for x, y in zip(b, b[1:]))) > 0       # ... in adjacent rows
        half = 1 << 29                                                         # a prefix sum that meets tau_q * S exactly
        assert sum(1 for v in q_of.values() if sum(v) and any((sum(v[:m]) << LWR_BITS) == half * sum(v) for m in range(1, len(v))))
        bad = np.nonzero(want["clade"] == CLADE_BAD_ROW)[0]                    # a bad row that is not the read's first
        assert sum(1 for i in bad if rows["branch"][i, 0] < rule.n) > 0
    if keep >= 16:
        assert sum(1 for v in q_of.values() if sum(v) << LWR_BITS >= 1 << 64) > 0     # S * 2^30 beyond uint64: it wraps
    # where keep rows of LWR 1.0 reach no threshold (S_m << 30 wraps below tau_q * S every time), a read of n_rows > keep
    # does so whose clade leaves branch 0 out: a prefix of n_rows rows, not of min(n_rows, keep), takes in rows that are
    # not the read's -- in the kernel the idle lanes of a group wider than keep, which hold branch 0 -- and another clade
    if rule.n >= 3 and keep & (keep - 1) and never_reached([1 << LWR_BITS] * keep, tq):
        assert sum(1 for i in q_of if n_rows[i] > keep and never_reached(q_of[i], tq) and rule.first[int(want["clade"][i])] > 0) > 0


@pytest.mark.parametrize("tq", FORGED_TAUS)
@pytest.mark.parametrize("keep", FORGED_KEEPS)
@pytest.mark.parametrize("tree_name", ["one_branch", "hand", "multifurcating", "star300", "synth500", "ladder2001"])
def test_host_mirror_equals_the_rule_bit_for_bit_on_forged_rows(host_bins, tmp_path, tree_name, keep, tq):
    from epik_amd.confidence import tau_q
    assert FORGED_TAUS == (0, tau_q(0.5), tau_q(0.95), tau_q(1))
    assert never_reached([1 << LWR_BITS] * 33, tau_q(0.95)) and never_reached([1 << LWR_BITS] * 63, tau_q(0.5))
    parent, lengths, rule = forged_tree(tree_name)
    n = 1000 if keep <= 16 else 300
    rows, n_rows, counts = forged_batch(np.random.default_rng([keep, len(parent)]), n, keep, len(parent))
    want = numpy_rule(rule, rows, n_rows, counts, tq)
    got = host_records(host_bins, tmp_path, rows, n_rows, counts, parent, lengths, tq)
    assert same_bits(got, want), np.nonzero(got != want)[0][:10]
    assert_every_case_occurs(rule, rows, n_rows, counts, tq, want)


def _walk_clade_counts(assigned, parent):
    out = [0] * len(parent)
    for b in range(len(parent)):
        node = b
        while node >= 0:
            out[node] += int(assigned[b])
            node = int(parent[node])
    return out


def test_both_files_written_and_read_back(host_bins, oracle_lib, small_case, tmp_path):
    from epik_amd import confidence
    tree, db = small_case
    rows, n_rows, counts = oracle_lib.Oracle.from_synth(db).place(*synth.pack_reads(_reads(db.kmer_size)), num_threads=0)
    n = len(n_rows)
    weights = np.random.default_rng(2).integers(0, 5, size=n).astype(np.uint32)
    tq = confidence.tau_q(0.95)
    write_input(tmp_path / "in.bin", rows, n_rows, counts, weights, tree.parent, tree.branch_length)
    run = subprocess.run([os.path.join(host_bins, "confidence_test"), "tsv", str(tq), str(tmp_path / "in.bin"),
                          str(tmp_path / "assign.tsv"), str(tmp_path / "clades.tsv")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    want = numpy_rule(RuleTree(tree.parent, tree.branch_length), rows, n_rows, counts, tq)
    sizes = confidence.subtree_sizes(tree.parent)
    assert np.array_equal(sizes, tree.subtree_num_nodes)
    # the Python writers give the same bytes
    names = [f"read_{i}" for i in range(n)]
    assert (tmp_path / "assign.tsv").read_bytes() == confidence.format_assign_tsv(names, want, sizes, tq).encode()
    assigned, classes = confidence.clade_counts(want, weights, db.num_branches)
    assert (tmp_path / "clades.tsv").read_bytes() == confidence.format_clades_tsv(assigned, classes, sizes, tq).encode()
    # ... and the files read back are the records
    back = confidence.read_assign_tsv(str(tmp_path / "assign.tsv"))
    assert back["tau_q"] == tq and back["records"] == n and back["names"] == names
    for i in range(n):
        clade = int(want["clade"][i])
        if clade in capi.CLADE_CLASSES:
            assert back["edge_num"][i] == capi.CLADE_CLASSES[clade] and back["clade_size"][i] == 0 and back["edpl"][i] == 0
        else:
            assert back["edge_num"][i] == clade and back["clade_size"][i] == sizes[clade]
    assert np.array_equal(back["edpl"].view(np.uint64), want["edpl"].view(np.uint64))            # %.17g round-trips a double
    assert np.allclose(back["clade_mass"], want["clade_mass_q"] / 2.0 ** 30, rtol=0, atol=5e-10)
    assert {"too_short", "no_hit"} <= set(x for x in back["edge_num"] if isinstance(x, str))
    clades = confidence.read_clades_tsv(str(tmp_path / "clades.tsv"))
    assert clades["records"] == int(weights.sum()) and clades["assigned"].tolist() == assigned.tolist()
    assert clades["clade_assigned"].tolist() == _walk_clade_counts(assigned, tree.parent)
    assert int(clades["clade_assigned"][-1]) == clades["assigned_records"] == int(assigned.sum())    # the root's clade is everything assigned
    assert (clades["too_short"], clades["no_hit"]) == (classes["too_short"], classes["no_hit"]) and clades["too_short"] > 0


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert "--assign" not in default and "--assign-mass" not in default
    assert epik.driver_command(**kw, assign=False, assign_mass=None) == default
    assert epik.driver_command(**kw, assign=True)[:-1] == default[:-1] + ["--assign"]
    both = epik.driver_command(**kw, assign=True, assign_mass=0.5, profile_only=True, strand="both")
    assert both[:-1] == default[:-1] + ["--strand", "both", "--profile-only", "--assign", "--assign-mass", "0.5"]
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, assign_mass=0.5)
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, assign=True, db_shard=2)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--assign " in out.stdout and "--assign-mass" in out.stdout
    for extra in (["--assign-mass", "0.5"], ["--assign", "--assign-mass", "1.5"], ["--assign", "--db-shard", "2"]):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", os.path.join(ROOT, "epik.py"), "-o", ROOT]
                             + extra + [os.path.join(ROOT, "epik.py")], capture_output=True, text=True)
        assert run.returncode == 2, (extra, run.stdout, run.stderr)


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
@pytest.mark.parametrize("extra,words", [
    (["--assign", "--db-shard", "2"], ("--assign", "--db-shard")),
    (["--db-shard=2", "--assign", "--profile-only"], ("--db-shard",)),
    (["--assign-mass", "0.5"], ("--assign-mass", "--assign")),
    (["--assign", "--assign-mass", "1.5"], ("--assign-mass", "[0, 1]")),
    (["--assign", "--assign-mass=-0.1"], ("--assign-mass", "[0, 1]")),
    (["--assign", "--assign-mass", "half"], ("--assign-mass",)),
])
def test_drivers_refuse_before_touching_anything(host_bins, tmp_path, binary, extra, words):
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q",
                          str(tmp_path / "none.fasta"), "-o", str(tmp_path)] + extra, capture_output=True, text=True)
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and all(w in run.stderr for w in words), run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_driver_help_names_both_flags(host_bins, binary):
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--assign " in out.stdout and "--assign-mass" in out.stdout


def test_confidence_symbols_exist_and_refuse_null():
    lib = capi.load()
    names = ("epik_amd_tree_create", "epik_amd_tree_destroy", "epik_amd_tree_info", "epik_amd_tree_build_host",
             "epik_amd_tree_lca_host", "epik_amd_confidence_device", "epik_amd_placer_confidence_reads",
             "epik_amd_placer_confidence_strands", "epik_amd_placer_confidence_frames", "epik_amd_placer_confidence_mates")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.CONFIDENCE.itemsize == 16 and capi.CONFIDENCE.fields["edpl"][1] == 8
    assert (capi.CLADE_TOO_NARROW, capi.CLADE_TOO_SHORT, capi.CLADE_NO_HIT, capi.CLADE_BAD_ROW) == (
        CLADE_TOO_NARROW, CLADE_TOO_SHORT, CLADE_NO_HIT, CLADE_BAD_ROW)
    out = ctypes.c_void_p(7)
    assert lib.epik_amd_tree_create(0, None, None, 3, ctypes.byref(out)) == capi.ERR_INVALID and not out.value
    assert lib.epik_amd_tree_create(0, None, None, 3, None) == capi.ERR_INVALID
    lib.epik_amd_tree_destroy(None)                         # (as free(NULL))
    assert lib.epik_amd_tree_info(None, None, None, None) == capi.ERR_INVALID and b"null tree" in lib.epik_amd_last_error()
    size = ctypes.c_uint64(0)
    assert lib.epik_amd_tree_build_host(None, None, 0, None, ctypes.byref(size)) == capi.ERR_INVALID
    assert lib.epik_amd_tree_build_host(None, None, 7, None, ctypes.byref(size)) == capi.OK and size.value == 32 + 7 * (16 + 8 * 3) + 32
    assert lib.epik_amd_tree_lca_host(None, None, None, 0, None) == capi.ERR_INVALID
    assert lib.epik_amd_confidence_device(None, None, None, None, 1, 7, 0, None, None) == capi.ERR_INVALID
    assert b"null tree" in lib.epik_amd_last_error()
    assert lib.epik_amd_placer_confidence_reads(None, None, None, 1, None, None, None, None, 0, None, None, None) == capi.ERR_INVALID
    for fn, mode in ((lib.epik_amd_placer_confidence_strands, capi.STRAND_BOTH), (lib.epik_amd_placer_confidence_frames, capi.FRAMES_BOTH),
                     (lib.epik_amd_placer_confidence_mates, capi.STRAND_FORWARD)):
        assert fn(None, None, None, 1, mode, None, None, None, None, None, 0, None, None, None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    # a tree that is valid needs a device to live on: no CPU fallback
    p, bl = np.array([2, 2, capi.TREE_NO_PARENT], np.uint32), np.ones(3)
    if capi.device_count() == 0:
        assert lib.epik_amd_tree_create(0, p.ctypes.data, bl.ctypes.data, 3, ctypes.byref(out)) == capi.ERR_NO_DEVICE
