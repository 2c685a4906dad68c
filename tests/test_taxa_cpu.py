"""Taxonomic assignment without a GPU (include/epik_amd.h: epik_amd_taxonomy): the hand values of the rule; the parser,
the numbering and the labeller -- Python mirror, host code (bin/taxa_test) and a brute-force labelling over parent walks
--; every parser, labeller and validation error by the line, leaf, taxon or branch it names; the rule over whole arrays
(epik_amd.taxonomy.numpy_assign: candidates from the id-sorted rows and their adjacent lcas) against the brute force
"mass(c) of EVERY taxon, the lowest that qualifies" on forged rows, which is the check of the candidate-closure
argument; every class and edge of the rule's arithmetic on those rows; the host mirror (epik_amd/host/taxonomy.cpp,
through the library's epik_amd_taxonomy_assign_host and through bin/taxa_test) against numpy bit for bit, records and
cells; the new symbols."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

try:  # torch first: its HIP runtime must be the process's before libepik_amd's loads (capi.check_hip_runtime)
    import torch  # noqa: F401
except ImportError:
    pass

from epik_amd import capi, synth, taxonomy
from test_assign_cpu import HAND_LENGTH, HAND_PARENT, RuleTree, caterpillar, forged_batch, hand_read, rule_record, star

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "epik_amd", "bin")
LWR_BITS = 30
TOO_NARROW = 0xFFFFFFFF
M64 = (1 << 64) - 1
SAT = 0xFFFFFFFF
U64 = np.uint64
CLASSES = (capi.TAXON_TOO_NARROW, capi.TAXON_TOO_SHORT, capi.TAXON_NO_HIT, capi.TAXON_BAD_ROW, capi.TAXON_NO_MASS)
FORGED_KEEPS = (1, 2, 3, 7, 8, 13, 64)
FORGED_TAUS = ((1 << 29) + 1, int(np.rint(0.95 * 2 ** 30)), 1 << 30)
FORGED_N = 199                                     # the branches of the forged rows: synth.make_tree(100)

# the hand case: the tree ((A,B)C,(D,E)F)R of test_assign_cpu and three ranks; E is the foreign leaf under F
HAND_NAMES = ["A", "B", "C", "D", "E", "F", "R"]
HAND_TAXONOMY = ("# leaf\ttaxopath\n"
                 "A\tBacteria;Proteo;Gamma\n"
                 "\n"
                 "B\tBacteria; Proteo ;Alpha\n"
                 "D\tBacteria;Firmi;Bacilli\n"
                 "  # the odd one out\n"
                 " E \tArchaea;Eury;Halo\r\n")
HAND_PATHS = ["Archaea;Eury;Halo", "Archaea;Eury", "Archaea", "Bacteria;Firmi;Bacilli", "Bacteria;Firmi", "Bacteria;Proteo;Alpha",
              "Bacteria;Proteo;Gamma", "Bacteria;Proteo", "Bacteria", ""]
HAND_TAXON_PARENT = [1, 2, 9, 4, 8, 7, 7, 8, 9, -1]
HAND_TAXON_FIRST = [0, 0, 0, 3, 3, 5, 6, 5, 3, 0]
HAND_LABEL = [6, 5, 7, 3, 0, 9, 9]                 # A Gamma, B Alpha, C Proteo, D Bacilli, E Halo, F the root (E is foreign), R


def q(x):
    """llrint(x * 2^30), round half to even."""
    return int(np.rint(np.float64(x) * np.float64(1 << LWR_BITS)))


@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


def parents_u32(parent):
    parent = np.asarray(parent).astype(np.int64)
    return np.where(parent < 0, capi.TREE_NO_PARENT, parent).astype(np.uint32)


def write_assign_input(path, rows, n_rows, counts, weights, samples, taxon_parent, label, num_samples):
    n, keep = rows.shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5Q", n, keep, len(label), len(taxon_parent), num_samples))
        fh.write(np.ascontiguousarray(rows, dtype=capi.PLACEMENT).tobytes())
        for a in (n_rows, counts, weights, samples):
            fh.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())
        fh.write(np.ascontiguousarray(parents_u32(taxon_parent)).tobytes())
        fh.write(np.ascontiguousarray(label, dtype=np.uint32).tobytes())


def binary_records(host_bins, tmp_path, rows, n_rows, counts, taxon_parent, label, tau_q):
    n = len(n_rows)
    write_assign_input(tmp_path / "in.bin", rows, n_rows, counts, np.ones(n, np.uint32), np.zeros(n, np.uint32), taxon_parent, label, 1)
    run = subprocess.run([os.path.join(host_bins, "taxa_test"), "records", str(tau_q), str(tmp_path / "in.bin"),
                          str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return np.fromfile(tmp_path / "out.bin", dtype=capi.TAXON_RECORD)


def binary_cells(host_bins, tmp_path, rows, n_rows, counts, weights, samples, taxon_parent, label, num_samples, tau_q):
    write_assign_input(tmp_path / "in.bin", rows, n_rows, counts, weights, samples, taxon_parent, label, num_samples)
    run = subprocess.run([os.path.join(host_bins, "taxa_test"), "cells", str(tau_q), str(tmp_path / "in.bin"),
                          str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    raw, S, T = np.fromfile(tmp_path / "out.bin", dtype=U64), num_samples, len(taxon_parent)
    assert len(raw) == 2 * S * T + 6 * S + 1
    return taxonomy.TaxaCells(raw[:S * T].reshape(S, T), raw[S * T:2 * S * T].reshape(S, T),
                              raw[2 * S * T:2 * S * T + 6 * S].copy().view(capi.TAXA_TOTALS), int(raw[-1]))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def hand_reads(keep=7):
    """Three reads on the hand tree: hand_read of --assign (A .5, B .25, D .25); D .4, A .3, B .3, where the prefix of
    the best rows and the lowest qualifying taxon part; F .7, E .3, an inner branch whose label is the root."""
    rows = np.zeros((3, keep), dtype=capi.PLACEMENT)
    rows["branch"][:] = 0xFFFFFFFF
    rows["lwr"][:] = np.nan
    rows[0] = hand_read(keep)[0][0]
    rows["branch"][1, :3], rows["lwr"][1, :3] = [3, 0, 1], [0.4, 0.3, 0.3]
    rows["branch"][2, :2], rows["lwr"][2, :2] = [5, 4], [0.7, 0.3]
    return rows, np.array([3, 3, 2], np.uint32), np.ones((3, keep), np.uint32)


def hand_expectations():
    """(tau, [(taxon, taxon_mass_q, first_taxon, total_q)] of the three reads), worked by hand."""
    one = 1 << 30
    s1 = q(0.4) + 2 * q(0.3)
    assert (q(0.3), q(0.4), q(0.7), s1, q(0.7) + q(0.3)) == (322122547, 429496730, 751619277, 1073741824, one)
    return [
        # Bacteria holds all of read 0, Proteo three quarters; read 1: Proteo .6, Bacteria all; read 2: only the root has .7
        (0.95, [(8, one, 6, one), (8, s1, 3, s1), (9, one, 9, one)]),
        # three quarters exactly: Proteo of read 0 meets it (mass * 2^30 == tau_q * S); read 2: still the root
        (0.75, [(7, 3 << 28, 6, one), (8, s1, 3, s1), (9, one, 9, one)]),
        # .55: Proteo of read 1 (.6), though its best row is D -- the prefix of the best rows D, A has the root for lca
        (0.55, [(7, 3 << 28, 6, one), (7, 2 * q(0.3), 3, s1), (9, one, 9, one)]),
    ]


def test_hand_values_in_numpy():
    taxa = taxonomy.parse_taxonomy(HAND_TAXONOMY)
    assert taxa.path == HAND_PATHS and taxa.parent.tolist() == HAND_TAXON_PARENT and taxa.first.tolist() == HAND_TAXON_FIRST
    assert taxa.leaf == ["A", "B", "D", "E"] and taxa.leaf_taxon == [6, 5, 3, 0] and taxa.leaf_line == [2, 4, 5, 7]
    label = taxonomy.label_branches(taxa, HAND_PARENT, HAND_NAMES)
    assert label.tolist() == HAND_LABEL
    rows, n_rows, counts = hand_reads()
    for tau, want in hand_expectations():
        tq = taxonomy.mass_tau_q(tau)
        records, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq)
        got = [tuple(int(x) for x in r) for r in records.tolist()]
        assert got == want, (tau, got)
        assert cells.totals["placed"][0] == 3 and cells.assigned[0].sum() == 3 and cells.bad_samples == 0
        direct = np.zeros(10, U64)
        for t, m in ((6, q(0.5) + q(0.3)), (5, q(0.25) + q(0.3)), (3, q(0.25) + q(0.4)), (9, q(0.7)), (0, q(0.3))):
            direct[t] = m
        assert np.array_equal(cells.direct[0], direct)
        # the clade sums: Bacteria holds reads 0 and 1 whole, the root everything
        clade = taxonomy.clade_sums(cells.direct, taxa.first)[0]
        assert int(clade[8]) == (1 << 30) + q(0.4) + 2 * q(0.3) and int(clade[9]) == int(direct.sum()) and int(clade[2]) == q(0.3)
    # where --assign's rule and this one part: the prefix D, A of read 1 has the root for lca, whose label is the root
    tree = RuleTree(HAND_PARENT, HAND_LENGTH)
    clade, _, _ = rule_record(tree, rows["branch"][1, :3], rows["lwr"][1, :3], 3, 1, 7, taxonomy.mass_tau_q(0.55))
    assert clade == 6 and HAND_LABEL[clade] == 9 != 7
    assert (taxonomy.mass_tau_q(0.95), taxonomy.mass_tau_q(1)) == (int(np.rint(0.95 * 2 ** 30)), 1 << 30)
    for bad in (0.5, 0.0, 1.5, -1):
        with pytest.raises(ValueError):
            taxonomy.mass_tau_q(bad)


def write_tree(path, parent, names):
    with open(path, "wb") as fh:
        fh.write(struct.pack("<Q", len(parent)))
        fh.write(np.ascontiguousarray(parents_u32(parent)).tobytes())
        for name in names:
            raw = name.encode()
            fh.write(struct.pack("<I", len(raw)) + raw)


def binary_labels(host_bins, tmp_path, text, parent, names):
    """(returncode, stdout, (taxon_parent, first, label, paths) or None) of `taxa_test labels`."""
    (tmp_path / "taxonomy.tsv").write_bytes(text.encode())
    write_tree(tmp_path / "tree.bin", parent, names)
    run = subprocess.run([os.path.join(host_bins, "taxa_test"), "labels", str(tmp_path / "taxonomy.tsv"), str(tmp_path / "tree.bin"),
                          str(tmp_path / "labels.bin")], capture_output=True, text=True)
    if run.returncode != 0:
        return run.returncode, run.stdout + run.stderr, None
    raw = (tmp_path / "labels.bin").read_bytes()
    T, = struct.unpack_from("<Q", raw, 0)
    at = 8
    taxon_parent = np.frombuffer(raw, np.uint32, T, at)
    first = np.frombuffer(raw, np.uint32, T, at + 4 * T)
    label = np.frombuffer(raw, np.uint32, len(parent), at + 8 * T)
    at += 8 * T + 4 * len(parent)
    paths = []
    for _ in range(T):
        length, = struct.unpack_from("<I", raw, at)
        paths.append(raw[at + 4:at + 4 + length].decode())
        at += 4 + length
    assert at == len(raw)
    return 0, run.stdout, (taxon_parent, first, label, paths)


def test_hand_values_through_the_host_mirror(host_bins, tmp_path):
    code, out, got = binary_labels(host_bins, tmp_path, HAND_TAXONOMY, HAND_PARENT, HAND_NAMES)
    assert code == 0, out
    taxon_parent, first, label, paths = got
    assert paths == HAND_PATHS and first.tolist() == HAND_TAXON_FIRST and label.tolist() == HAND_LABEL
    assert taxon_parent.tolist() == parents_u32(HAND_TAXON_PARENT).tolist()
    rows, n_rows, counts = hand_reads()
    for tau, want in hand_expectations():
        tq = taxonomy.mass_tau_q(tau)
        for records in (binary_records(host_bins, tmp_path, rows, n_rows, counts, HAND_TAXON_PARENT, HAND_LABEL, tq),
                        taxonomy.assign_host(HAND_TAXON_PARENT, HAND_LABEL, rows, n_rows, counts, tq)[0]):
            assert [tuple(int(x) for x in r) for r in records.tolist()] == want, tau


def random_tree(n, rng):
    """parent[] of a random rooted tree of n nodes in post-order ids, multifurcations and unary nodes included."""
    above = [-1] + [int(rng.integers(0, k)) for k in range(1, n)]          # node k hangs below an earlier node
    kids = [[] for _ in range(n)]
    for k in range(1, n):
        kids[above[k]].append(k)
    order, stack = [], [(0, 0)]
    while stack:
        node, at = stack.pop()
        if at < len(kids[node]):
            stack.append((node, at + 1))
            stack.append((kids[node][at], 0))
        else:
            order.append(node)
    new_id = {old: new for new, old in enumerate(order)}
    parent = np.full(n, -1, np.int64)
    for k in range(1, n):
        parent[new_id[k]] = new_id[above[k]]
    return parent


def leaves_of(parent):
    inner = set(int(p) for p in parent if p >= 0)
    return [b for b in range(len(parent)) if b not in inner]


def random_taxonomy_text(parent, rng, kind):
    """A taxonomy file for the leaves L<b> of the tree: `random` paths out of a small trie, the `root` alone, or
    prefixes of a `chain` 40 deep."""
    lines = []
    for b in leaves_of(parent):
        if kind == "root":
            path = "-"
        elif kind == "chain":
            path = ";".join(f"c{d}" for d in range(int(rng.integers(1, 41)) if b else 40))
        else:
            depth = int(rng.integers(0, 4))
            path = ";".join(f"{'xyz'[d]}{int(rng.integers(0, 3))}" for d in range(depth)) or "-"
        lines.append(f"L{b}\t{path}")
    rng.shuffle(lines)
    return "\n".join(lines) + "\n"


def brute_labels(taxa, parent, names):
    """label[b] = the taxon of the longest common prefix of the taxopaths of the leaves found below b by parent walks."""
    path_of = {name: taxa.path[t] for name, t in zip(taxa.leaf, taxa.leaf_taxon)}
    below = [[] for _ in parent]
    for leaf in leaves_of(parent):
        node = leaf
        while node >= 0:
            below[node].append(leaf)
            node = int(parent[node])
    taxon_of = {p: t for t, p in enumerate(taxa.path)}
    out = []
    for b in range(len(parent)):
        lists = [path_of[names[leaf]].split(";") if path_of[names[leaf]] else [] for leaf in below[b]]
        common = []
        for column in zip(*lists):
            if len(set(column)) != 1:
                break
            common.append(column[0])
        out.append(taxon_of[";".join(common)])
    return out


LABEL_CASES = [(n, kind) for n in (1, 2, 7, 200) for kind in ("random", "root", "chain")] + [(n, "synth") for n in (1, 7, 199)]


@pytest.mark.parametrize("n,kind", LABEL_CASES)
def test_parser_and_labeller_agree_with_brute_force(host_bins, tmp_path, n, kind):
    rng = np.random.default_rng([n, len(kind)])
    if kind == "synth":
        tree = synth.make_tree((n + 1) // 2, seed=n)
        parent, names = tree.parent, tree.labels
        text = synth.synth_taxonomy(tree, 4, seed=n + 1)
    else:
        parent = random_tree(n, rng)
        names = [f"L{b}" for b in range(n)]
        text = random_taxonomy_text(parent, rng, kind)
    taxa = taxonomy.parse_taxonomy(text)
    T = taxa.num_taxa
    # the conventions of epik_amd_tree: post-order ids, the root last, children in bytewise order of their names
    assert taxa.parent[-1] == -1 and (taxa.parent[:-1] > np.arange(T - 1)).all() and taxa.path[-1] == ""
    assert np.array_equal(taxa.first, taxonomy.taxonomy_first(taxa.parent)) and len(set(taxa.path)) == T
    for t in range(T - 1):
        assert taxa.path[t].rsplit(";", 1)[0] == taxa.path[taxa.parent[t]] or (";" not in taxa.path[t] and taxa.parent[t] == T - 1)
    for p in range(T):
        kids = [taxa.path[t].encode() for t in range(T - 1) if taxa.parent[t] == p]
        assert kids == sorted(kids)
    if kind == "root":
        assert T == 1
    if kind == "chain":
        assert T == 41 and (taxa.parent[:-1] == np.arange(1, 41)).all()
    label = taxonomy.label_branches(taxa, parent, names)
    assert label.tolist() == brute_labels(taxa, parent, names)
    if kind in ("random", "synth") and n >= 199:
        inner = sorted(set(range(n)) - set(leaves_of(parent)))
        assert (label[inner] == T - 1).sum() > 1 and (label[inner] != T - 1).sum() > 1      # some back off to the root, not all
        assert len(set(np.bincount(parent[parent >= 0]))) > 2 or kind == "synth"                # a multifurcation
    code, out, got = binary_labels(host_bins, tmp_path, text, parent, names)
    assert code == 0, out
    assert got[0].tolist() == taxa.parents().tolist() and got[1].tolist() == taxa.first.tolist()
    assert got[2].tolist() == label.tolist() and got[3] == taxa.path
    # the library takes what the parser gives
    rows = np.zeros((1, 1), dtype=capi.PLACEMENT)
    records, _ = taxonomy.assign_host(taxa.parent, label, rows, np.ones(1, np.uint32), np.ones((1, 1), np.uint32), 1 << 30)
    assert int(records["taxon"][0]) == capi.TAXON_NO_MASS


PARSER_ERRORS = [
    ("A\tx;y\nB x;y\n", "line 2:", "tab"),
    ("A\tx;y\n\n# c\nB\tx;;y\n", "line 4:", "empty element"),
    ("A\tx;y\nB\t\n", "line 2:", "empty element"),
    ("A\tx;y\nB\tx; ;z\n", "line 2:", "empty element"),
    ("A\tx;y;\n", "line 1:", "empty element"),
    ("A\tx\nB\ty\n#\nA\tz\n", "line 4:", "twice"),
    ("\tx\n", "line 1:", "leaf label"),
]


@pytest.mark.parametrize("text,names_line,word", PARSER_ERRORS)
def test_every_parser_error_names_its_line(host_bins, tmp_path, text, names_line, word):
    with pytest.raises(taxonomy.TaxonomyError) as e:
        taxonomy.parse_taxonomy(text)
    assert str(e.value).startswith(names_line) and word in str(e.value)
    code, out, _ = binary_labels(host_bins, tmp_path, text, [1, -1], ["A", "R"])
    assert code == 1 and out.startswith(names_line) and word in out, out


def test_labeller_errors_name_the_leaf_or_the_line(host_bins, tmp_path):
    cases = [("A\tx\nB\ty\nD\tz\n", "leaf E:"),                  # a tree leaf the file does not give
             ("A\tx\nB\ty\nD\tz\nE\tz\n\nC\tx\n", "line 6:"),     # an inner branch's name is no leaf
             ("A\tx\nQ\tx\nB\ty\nD\tz\nE\tz\n", "line 2:")]       # a label that is not in the tree
    for text, names in cases:
        taxa = taxonomy.parse_taxonomy(text)
        with pytest.raises(taxonomy.TaxonomyError) as e:
            taxonomy.label_branches(taxa, HAND_PARENT, HAND_NAMES)
        assert str(e.value).startswith(names), str(e.value)
        code, out, _ = binary_labels(host_bins, tmp_path, text, HAND_PARENT, HAND_NAMES)
        assert code == 1 and out.startswith(names), out


INVALID_TAXONOMIES = [
    # (taxon_parent, label, what the message begins with)
    ([0, 2, -1], [0], "taxon 0:"),                  # a parent not above its child
    ([2, 3, -1], [0], "taxon 1:"),                  # ... outside the taxonomy
    ([2, -1, -1], [0], "taxon 1:"),                 # a second root
    ([2, 2, 1], [0], "taxon 2:"),                   # the last taxon with a parent
    ([2, 3, 3, -1], [0], "taxon 2:"),               # descendants that are not [first, t]
    ([2, 2, -1], [0, 1, 3, 2], "branch 2:"),        # a label that is no taxon
]


@pytest.mark.parametrize("taxon_parent,label,begins", INVALID_TAXONOMIES)
def test_every_validation_error_names_its_taxon_or_branch(host_bins, tmp_path, taxon_parent, label, begins):
    rows = np.zeros((1, 2), dtype=capi.PLACEMENT)
    with pytest.raises(capi.EpikAmdError) as e:
        taxonomy.assign_host(taxon_parent, label, rows, np.ones(1, np.uint32), np.ones((1, 2), np.uint32), 1 << 30)
    message = str(e.value).split(": ", 1)[1]
    assert e.value.code == capi.ERR_INVALID and message.startswith(begins), message
    if begins.startswith("taxon"):
        assert "branch" not in message
        # the host code's own validator (taxonomy.cpp, built without the library) refuses in the same words
        write_assign_input(tmp_path / "in.bin", rows, np.ones(1, np.uint32), np.ones((1, 2), np.uint32), np.ones(1, np.uint32),
                           np.zeros(1, np.uint32), taxon_parent, label, 1)
        run = subprocess.run([os.path.join(host_bins, "taxa_test"), "records", str(1 << 30), str(tmp_path / "in.bin"),
                              str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert run.returncode == 1 and run.stdout.strip() == message, (run.stdout, message)


def taxonomy_shapes():
    """name -> (taxon_parent with -1 for the root, label[FORGED_N]) of the taxonomies the forged rows are assigned in: a
    caterpillar (deep chains of clades), a star (every taxon a child of the root), the root alone, and synth_taxonomy
    over the tree the branches belong to; the first three with labels drawn at random -- the rule takes any label[]."""
    rng = np.random.default_rng(99)
    out = {}
    for name, parent in (("caterpillar", caterpillar(101)[0]), ("star", star(60)[0]), ("root", np.array([-1]))):
        out[name] = (np.asarray(parent, dtype=np.int64), rng.integers(0, len(parent), size=FORGED_N).astype(np.uint32))
    tree = synth.make_tree((FORGED_N + 1) // 2, seed=13)
    taxa = taxonomy.parse_taxonomy(synth.synth_taxonomy(tree, 4, seed=14))
    out["synth"] = (taxa.parent, taxonomy.label_branches(taxa, tree.parent, tree.labels))
    assert tree.num_nodes == FORGED_N and taxa.num_taxa > 40
    return out


SHAPES = taxonomy_shapes()
_BATCHES = {}


def forged(keep):
    """The forged batch of a keep, made once."""
    if keep not in _BATCHES:
        _BATCHES[keep] = forged_batch(np.random.default_rng([keep, FORGED_N]), 4096, keep, FORGED_N)
    return _BATCHES[keep]


def brute_force(taxon_parent, label, rows, n_rows, counts):
    """What the rule looks at, read by read, and mass(c) of EVERY taxon c: (cls [n], t, q as lists per read, total [n],
    mass float64 [n][T] -- sums of at most 64 integers below 2^31, exact in a double)."""
    n, keep = rows.shape
    T, N = len(taxon_parent), len(label)
    above = np.zeros((T, T))                                   # above[c, t] = 1: c is t or an ancestor of t
    for t in range(T):
        c = t
        while c >= 0:
            above[c, t] = 1.0
            c = int(taxon_parent[c])
    cls, ts, qs, direct = np.zeros(n, np.int64), [], [], np.zeros((n, T))
    for i in range(n):
        t_i, q_i = [], []
        if n_rows[i] == TOO_NARROW:
            cls[i] = capi.TAXON_TOO_NARROW
        elif n_rows[i] == 0:
            cls[i] = capi.TAXON_TOO_SHORT
        elif counts[i, 0] == 0:
            cls[i] = capi.TAXON_NO_HIT
        else:
            nr = min(int(n_rows[i]), keep)
            if any(int(b) >= N for b in rows["branch"][i, :nr]):
                cls[i] = capi.TAXON_BAD_ROW
            else:
                t_i = [int(label[b]) for b in rows["branch"][i, :nr]]
                q_i = [q(x) for x in rows["lwr"][i, :nr]]
                if sum(q_i) == 0:
                    cls[i] = capi.TAXON_NO_MASS
                else:
                    for t, m in zip(t_i, q_i):
                        direct[i, t] += m
        ts.append(t_i), qs.append(q_i)
    total = np.array([sum(v) for v in qs], dtype=np.int64)
    return cls, ts, qs, total, direct @ above.T


def brute_records(brute, tau_q, wrapping=False):
    """The records from mass(c) of every taxon: the lowest id with mass * 2^30 >= tau_q * S, on Python ints (wrapping:
    both sides taken modulo 2^64, as the confidence rule compares -- what this rule must NOT do)."""
    cls, ts, qs, total, mass = brute
    out = np.zeros(len(cls), dtype=capi.TAXON_RECORD)
    out["taxon"] = cls
    for i in np.nonzero(cls == 0)[0]:
        S = int(total[i])
        need = tau_q * S
        for c in np.nonzero(mass[i])[0]:
            m = int(mass[i, c])
            if (((m << LWR_BITS) & M64) >= (need & M64)) if wrapping else ((m << LWR_BITS) >= need):
                out[i] = (c, min(m, SAT), ts[i][0], min(S, SAT))
                break
        else:
            assert wrapping
            out[i] = (SAT, 0, ts[i][0], min(S, SAT))
    return out


@pytest.mark.parametrize("keep", FORGED_KEEPS)
def test_rule_equals_brute_force_and_every_case_occurs(keep):
    rows, n_rows, counts = forged(keep)
    seen = dict(exact=0, beyond=0, wrap_differs=0, sat_mass=0, sat_total=0, closure=0)
    for name, (taxon_parent, label) in SHAPES.items():
        brute = brute_force(taxon_parent, label, rows, n_rows, counts)
        cls, ts, qs, total, mass = brute
        # every class occurs, and the placed reads are many
        assert all((cls == c).sum() > 0 for c in CLASSES) and (cls == 0).sum() > 4096 // 4, name
        assert ((n_rows > keep) & (n_rows != TOO_NARROW) & (cls == 0)).sum() > 0                 # n_rows beyond keep: clamped
        for tq in FORGED_TAUS:
            want = brute_records(brute, tq)
            got, _ = taxonomy.numpy_assign(taxon_parent, label, rows, n_rows, counts, tq)
            assert same_bits(got, want), (name, tq, np.nonzero(got != want)[0][:10])
            placed = want["taxon"] < len(taxon_parent)
            assert np.array_equal(placed, cls == 0) and not want["taxon_mass_q"][~placed].any() and not want["total_q"][~placed].any()
            seen["sat_mass"] += int((want["taxon_mass_q"] == SAT).sum())
            seen["sat_total"] += int((want["total_q"] == SAT).sum())
            root = len(taxon_parent) - 1
            for i in np.nonzero(placed)[0]:
                m, S, c = int(mass[i, want["taxon"][i]]), int(total[i]), int(want["taxon"][i])
                # a comparison met exactly, below the root, by a read of several taxa
                seen["exact"] += (m << LWR_BITS) == tq * S and c != root and len(set(ts[i])) > 1
                # the taxon is none of the rows' own: an lca of two of them
                seen["closure"] += c not in ts[i]
            big = placed & (total >= 1 << 34)
            seen["beyond"] += int(big.sum())
            if big.any():
                wrapped = brute_records(brute, tq, wrapping=True)
                seen["wrap_differs"] += int((wrapped["taxon"][big] != want["taxon"][big]).sum())
    assert seen["exact"] > 0 or keep == 1, seen
    if keep > 1:
        assert seen["closure"] > 0, seen
    if keep >= 7:                                   # all LWRs 1.0 on four rows or more: both 32-bit fields saturate
        assert seen["sat_mass"] > 0 and seen["sat_total"] > 0, seen
    if keep >= 16:                                  # S * 2^30 beyond uint64: a comparison that wraps gives another taxon
        assert seen["beyond"] > 0 and seen["wrap_differs"] > 0, seen


def forged_weights_and_samples(n, num_samples, rng):
    """Weights with 0 and 2^32 - 1; samples in runs, then a stretch interleaved, some of no sample, one sample empty."""
    weights = rng.integers(0, 5, size=n).astype(np.uint32)
    weights[::11] = 0
    weights[5::13] = 0xFFFFFFFF
    cuts = np.sort(rng.integers(0, n, size=num_samples - 2))
    samples = np.searchsorted(cuts, np.arange(n), side="right").astype(np.uint32)      # runs over 0 .. S - 2
    samples[n // 2:n // 2 + 300] = rng.integers(0, num_samples - 1, size=300)          # interleaved
    empty = num_samples // 2
    samples[samples >= empty] += 1                                                      # sample `empty` has no read
    samples[3::97] = num_samples + 5
    samples[n - 1] = 0xFFFFFFFF
    return weights, samples, empty


@pytest.mark.parametrize("keep", FORGED_KEEPS)
def test_host_mirror_equals_numpy_bit_for_bit(host_bins, tmp_path, keep):
    rows, n_rows, counts = forged(keep)
    n, S = len(n_rows), 5
    weights, samples, empty = forged_weights_and_samples(n, S, np.random.default_rng(keep))
    for name, (taxon_parent, label) in SHAPES.items():
        for tq in FORGED_TAUS:
            want, cells = taxonomy.numpy_assign(taxon_parent, label, rows, n_rows, counts, tq, weights, samples, S)
            got, got_cells = taxonomy.assign_host(taxon_parent, label, rows, n_rows, counts, tq, weights, samples, S)
            assert same_bits(got, want), (name, tq, np.nonzero(got != want)[0][:10])
            assert got_cells.same_as(cells), (name, tq)
            assert cells.bad_samples == int((samples >= S).sum()) > 2
            assert not cells.direct[empty].any() and not cells.assigned[empty].any() and not cells.totals[empty:empty + 1].view(U64).any()
            assert all(cells.totals[k].sum() > 0 for k in taxonomy.TOTALS)
            placed = want["taxon"] < len(taxon_parent)
            known = samples < S
            assert int(cells.assigned.sum(dtype=U64)) == int(cells.totals["placed"].sum(dtype=U64)) == int(weights[placed & known].astype(U64).sum(dtype=U64))
            if tq == FORGED_TAUS[1] and name in ("synth", "caterpillar"):
                # the stand-alone binary: the same code without the library
                assert same_bits(binary_records(host_bins, tmp_path, rows, n_rows, counts, taxon_parent, label, tq), want)
                assert binary_cells(host_bins, tmp_path, rows, n_rows, counts, weights, samples, taxon_parent, label, S, tq).same_as(cells)
    # no weights and no samples: every read once, into the only row; the cells are added to what is there
    taxon_parent, label = SHAPES["synth"]
    want, cells = taxonomy.numpy_assign(taxon_parent, label, rows, n_rows, counts, 1 << 30)
    got, got_cells = taxonomy.assign_host(taxon_parent, label, rows, n_rows, counts, 1 << 30)
    assert same_bits(got, want) and got_cells.same_as(cells) and cells.bad_samples == 0
    assert sum(int(cells.totals[k][0]) for k in taxonomy.TOTALS) == n
    only_records, none = taxonomy.assign_host(taxon_parent, label, rows, n_rows, counts, 1 << 30, want_cells=False)
    assert none is None and same_bits(only_records, want)
    none, only_cells = taxonomy.assign_host(taxon_parent, label, rows, n_rows, counts, 1 << 30, want_records=False)
    assert none is None and only_cells.same_as(cells)


def test_taxonomy_symbols_exist_and_refuse_nulls():
    lib = capi.load()
    names = ("epik_amd_taxonomy_create", "epik_amd_taxonomy_destroy", "epik_amd_taxonomy_reset", "epik_amd_taxonomy_info",
             "epik_amd_taxonomy_read", "epik_amd_taxonomy_add_cells", "epik_amd_taxonomy_add_device", "epik_amd_taxonomy_assign_host")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert capi.ABI_VERSION == 3 and capi.TAXON_RECORD.itemsize == 16 and capi.TAXA_TOTALS.itemsize == 48
    assert (capi.TAXON_TOO_NARROW, capi.TAXON_TOO_SHORT, capi.TAXON_NO_HIT, capi.TAXON_BAD_ROW) == (
        capi.CLADE_TOO_NARROW, capi.CLADE_TOO_SHORT, capi.CLADE_NO_HIT, capi.CLADE_BAD_ROW) and capi.TAXON_NO_MASS == 0xFFFFFFFB
    err = lambda: lib.epik_amd_last_error().decode()
    out = ctypes.c_void_p(7)
    parent, label = np.array([capi.TREE_NO_PARENT], np.uint32), np.zeros(3, np.uint32)
    assert lib.epik_amd_taxonomy_create(None, parent.ctypes.data, 1, label.ctypes.data, 1, ctypes.byref(out)) == capi.ERR_INVALID
    assert not out.value and "null placer" in err()
    assert lib.epik_amd_taxonomy_create(None, None, 1, None, 1, None) == capi.ERR_INVALID
    lib.epik_amd_taxonomy_destroy(None)                         # (as free(NULL))
    for call in (lambda: lib.epik_amd_taxonomy_reset(None), lambda: lib.epik_amd_taxonomy_info(None, None, None, None, None),
                 lambda: lib.epik_amd_taxonomy_read(None, None, None, None, None),
                 lambda: lib.epik_amd_taxonomy_add_cells(None, None, None, None),
                 lambda: lib.epik_amd_taxonomy_add_device(None, None, None, None, None, None, 1, 1 << 30, None, None)):
        assert call() == capi.ERR_INVALID and "null taxonomy" in err()
    host = lambda tq, p=parent.ctypes.data, lab=label.ctypes.data, keep=7: lib.epik_amd_taxonomy_assign_host(
        p, 1, lab, 3, keep, None, None, None, None, None, 1, 1, tq, None, None, None, None, None)
    assert host(1 << 30) == capi.ERR_INVALID and "null argument" in err()          # rows of one read, and none given
    assert host(1 << 30, p=None) == capi.ERR_INVALID and "null argument" in err()
    for tq in (0, 1 << 29, (1 << 30) + 1, 0xFFFFFFFF):
        assert host(tq) == capi.ERR_INVALID and "tau_q" in err(), tq
    assert host(1 << 30, keep=0) == capi.ERR_INVALID and host(1 << 30, keep=65) == capi.ERR_INVALID and "keep" in err()
    # cells: all four or none
    direct = np.zeros(1, U64)
    assert lib.epik_amd_taxonomy_assign_host(parent.ctypes.data, 1, label.ctypes.data, 3, 7, None, None, None, None, None, 0, 1,
                                             1 << 30, None, direct.ctypes.data, None, None, None) == capi.ERR_INVALID
    assert "all four" in err()
    # nothing to do is no error
    assert lib.epik_amd_taxonomy_assign_host(parent.ctypes.data, 1, label.ctypes.data, 3, 7, None, None, None, None, None, 0, 1,
                                             1 << 30, None, None, None, None, None) == capi.OK


def test_the_three_files_are_the_same_bytes_from_both_writers(host_bins, tmp_path):
    """taxa.tsv, taxa_reads.tsv and cohort_taxa.tsv as taxonomy.cpp and epik_amd/taxonomy.py format them, on forged rows
    (every class word occurs) over synth_taxonomy; the clade columns against a walk up the parents."""
    keep, S = 7, 5
    rows, n_rows, counts = (a[:600] for a in forged(keep))
    tree = synth.make_tree((FORGED_N + 1) // 2, seed=13)
    text = synth.synth_taxonomy(tree, 4, seed=14)
    taxa = taxonomy.parse_taxonomy(text)
    label = taxonomy.label_branches(taxa, tree.parent, tree.labels)
    weights, samples, empty = forged_weights_and_samples(600, S, np.random.default_rng(3))
    tq = taxonomy.mass_tau_q(0.95)
    records, cells = taxonomy.numpy_assign(taxa.parent, label, rows, n_rows, counts, tq, weights, samples, S)
    (tmp_path / "taxonomy.tsv").write_bytes(text.encode())
    write_assign_input(tmp_path / "in.bin", rows, n_rows, counts, weights, samples, taxa.parent, label, S)
    run = subprocess.run([os.path.join(host_bins, "taxa_test"), "files", str(tq), str(tmp_path / "in.bin"), str(tmp_path / "taxonomy.tsv"),
                          str(tmp_path) + os.sep], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    one = taxonomy.format_taxa_tsv(cells.direct[0], cells.assigned[0], cells.totals[0], taxa, tq)
    reads = taxonomy.format_taxa_reads_tsv([f"read_{i}" for i in range(600)], records, taxa, tq)
    cohort = taxonomy.format_cohort_taxa_tsv([f"sample_{s}" for s in range(S)], cells, taxa, tq)
    assert (tmp_path / "taxa.tsv").read_bytes() == one.encode()
    assert (tmp_path / "taxa_reads.tsv").read_bytes() == reads.encode()
    assert (tmp_path / "cohort_taxa.tsv").read_bytes() == cohort.encode()
    for word in ("too_short", "no_hit", "too_narrow", "no_mass", "bad_row"):
        assert f"\t0\t{word}\t-\n" in reads
    assert one.startswith(f"# epik_amd taxa v1\ttau_q={tq}\ttaxa={taxa.num_taxa}\n# records=") and "\t-\n" in one
    assert f"sample_{empty}\t" not in cohort and "sample_0\t" in cohort
    # the clade columns of sample 0: every taxon's cells summed up the parents
    want_a, want_m = [0] * taxa.num_taxa, [0] * taxa.num_taxa
    for t in range(taxa.num_taxa):
        c = t
        while c >= 0:
            want_a[c] = (want_a[c] + int(cells.assigned[0, t])) & M64
            want_m[c] = (want_m[c] + int(cells.direct[0, t])) & M64
            c = int(taxa.parent[c])
    body = [line.split("\t") for line in one.split("\n")[3:] if line]
    by_path = {("" if f[6] == "-" else f[6]): f for f in body}
    assert len(body) == sum(1 for a, m in zip(want_a, want_m) if a or m) > 5
    for t in range(taxa.num_taxa):
        if want_a[t] or want_m[t]:
            f = by_path[taxa.path[t]]
            assert (int(f[0]), int(f[1]), int(f[2]), int(f[3])) == (int(cells.assigned[0, t]), int(want_a[t]), int(cells.direct[0, t]), int(want_m[t]))
    fields = [line.split("\t") for line in reads.split("\n")[2:] if line]
    shares = [float(f[1]) for f in fields if f[2] not in capi.TAXON_CLASSES.values()]
    assert len(fields) == 600 and len(shares) > 150 and all(0.5 < x <= 1.0 for x in shares) and any(x == 1.0 for x in shares)


def test_host_entry_symbols_exist_and_refuse_nulls():
    lib = capi.load()
    names = ("epik_amd_placer_taxa_reads", "epik_amd_placer_taxa_strands", "epik_amd_placer_taxa_frames", "epik_amd_placer_taxa_mates")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert lib.epik_amd_placer_taxa_reads(None, None, None, 1, None, None, None, None, 1 << 30, None, None, None, None, None) == capi.ERR_INVALID
    assert b"null placer" in lib.epik_amd_last_error()
    for fn, mode in ((lib.epik_amd_placer_taxa_strands, capi.STRAND_BOTH), (lib.epik_amd_placer_taxa_frames, capi.FRAMES_BOTH),
                     (lib.epik_amd_placer_taxa_mates, capi.STRAND_FORWARD)):
        assert fn(None, None, None, 1, mode, None, None, None, None, None, 1 << 30, None, None, None, None, None) == capi.ERR_INVALID
        assert b"null placer" in lib.epik_amd_last_error()


def test_host_taxonomy_under_asan_ubsan(host_bins):
    """A stand-alone program over taxonomy.cpp built with -fsanitize=address,undefined: the parser and its errors, the
    labeller and its errors, the rule on the hand case and on forged batches at keep 1, 7 and 64.  Nothing is preloaded."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-taxa"], check=True, stdout=subprocess.DEVNULL)
    run = subprocess.run([os.path.join(host_bins, "san", "taxa_selftest_asan")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_launcher_passes_the_taxonomy_flags_only_when_given():
    import sys

    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="q.fasta")
    default = epik.driver_command(**kw)
    assert not any("taxonomy" in a for a in default)
    assert epik.driver_command(**kw, taxonomy=None, taxonomy_mass=None, taxonomy_per_read=False) == default
    assert epik.driver_command(**kw, taxonomy="t.tsv")[:-1] == default[:-1] + ["--taxonomy", "t.tsv"]
    full = epik.driver_command(**kw, taxonomy="t.tsv", taxonomy_mass=0.75, taxonomy_per_read=True, profile_only=True, strand="both")
    assert full[:-1] == default[:-1] + ["--strand", "both", "--profile-only", "--taxonomy", "t.tsv", "--taxonomy-mass", "0.75",
                                        "--taxonomy-per-read"]
    with_cohort = epik.driver_command(**kw, taxonomy="t.tsv", cohort=True, cohort_squash=True)
    assert with_cohort[:-1] == default[:-1] + ["--cohort", "--cohort-squash", "--taxonomy", "t.tsv"]
    for bad in (dict(taxonomy_mass=0.9), dict(taxonomy_per_read=True), dict(taxonomy="t.tsv", assign=True),
                dict(taxonomy="t.tsv", db_shard=2), dict(taxonomy="t.tsv", taxonomy_mass=0.5), dict(taxonomy="t.tsv", taxonomy_mass=1.5)):
        with pytest.raises(click.UsageError):
            epik.driver_command(**kw, **bad)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and all(f in out.stdout for f in ("--taxonomy ", "--taxonomy-mass", "--taxonomy-per-read"))
    for extra in (["--taxonomy-mass", "0.9"], ["--taxonomy-per-read"], ["--taxonomy", "t.tsv", "--assign"],
                  ["--taxonomy", "t.tsv", "--db-shard", "2"], ["--taxonomy", "t.tsv", "--taxonomy-mass", "0.5"]):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "epik.py"), "place", "-i", os.path.join(ROOT, "epik.py"), "-o", ROOT]
                             + extra + [os.path.join(ROOT, "epik.py")], capture_output=True, text=True)
        assert run.returncode == 2, (extra, run.stdout, run.stderr)


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
@pytest.mark.parametrize("extra,words", [
    (["--taxonomy-mass", "0.9"], ("--taxonomy-mass", "--taxonomy")),
    (["--taxonomy-per-read"], ("--taxonomy-per-read", "--taxonomy")),
    (["--taxonomy", "t.tsv", "--assign"], ("--taxonomy", "--assign")),
    (["--taxonomy", "t.tsv", "--db-shard", "2"], ("--taxonomy", "--db-shard")),
    (["--taxonomy=t.tsv", "--db-shard=2", "--profile-only"], ("--db-shard",)),
    (["--taxonomy", "t.tsv", "--taxonomy-mass", "0.5"], ("--taxonomy-mass", "(0.5, 1]")),
    (["--taxonomy", "t.tsv", "--taxonomy-mass", "1.01"], ("--taxonomy-mass", "(0.5, 1]")),
    (["--taxonomy", "t.tsv", "--taxonomy-mass", "most"], ("--taxonomy-mass",)),
    (["--taxonomy", "TAXONOMY_WITH_AN_ERROR"], ("line 2:", "empty element")),
    (["--taxonomy", "none.tsv"], ("none.tsv",)),
])
def test_drivers_refuse_before_touching_anything(host_bins, tmp_path, binary, extra, words):
    work = tmp_path / "work"
    work.mkdir()
    (tmp_path / "bad.tsv").write_text("A\tx;y\nB\tx;;y\n")
    extra = [str(tmp_path / "bad.tsv") if a == "TAXONOMY_WITH_AN_ERROR" else a for a in extra]
    run = subprocess.run([os.path.join(host_bins, binary), "-d", str(work / "none.ekdb"), "-q", str(work / "none.fasta"), "-o", str(work)]
                         + extra, capture_output=True, text=True, cwd=str(work))
    assert run.returncode == 255, run.stdout + run.stderr
    assert run.stderr.startswith("Error:") and all(w in run.stderr for w in words), run.stderr
    assert "Loading database" not in run.stdout and "HIP device" not in run.stderr
    assert not list(work.iterdir())


@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_driver_help_names_the_three_flags(host_bins, binary):
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and all(f in out.stdout for f in ("--taxonomy arg", "--taxonomy-mass", "--taxonomy-per-read"))
