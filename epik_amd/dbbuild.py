"""From files to a database: what `epik.py extend` and `epik.py build` do (host Python around epik_amd.build.Builder).

extend   the reference tree with ghost nodes and the alignment with their all-gap rows: what an ancestral
         reconstruction (RAxML-NG --ancestral, PhyML) is run on.
build    the reconstruction's posteriors of the ghost nodes, streamed into the device builder, to an .ekdb file.

ASSUMPTION (the tools are not available here; DESIGN.md's assumption register): the posterior file is the
tab-separated table RAxML-NG documents for --ancestral (*.ancestralProbs: a header, a `Node` and a `Site` column, 1-based
sites, one `p_<X>` column a state), and the tree it writes back (*.ancestralTree) carries the same node names as inner
labels.  `read_ar_header` / `ghost_posteriors` are the only code that knows that layout.
"""
from __future__ import annotations

import os

import numpy as np

from . import alphabet, newick

GHOST_PREFIX = "ghost_"
GHOST_LEAF_LENGTH = 0.01
GAP_CHARS = "-.?"


class BuildInputError(ValueError):
    pass


# ---- reading ------------------------------------------------------------------------------------------------------

def read_fasta(path: str) -> list:
    """[(name, sequence)] in file order; the name is the header's first word."""
    records, name, parts = [], None, []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                if name is not None:
                    records.append((name, "".join(parts)))
                words = line[1:].split()
                if not words:
                    raise BuildInputError(f"{path}, line {number}: a record without a name")
                name, parts = words[0], []
            elif line.strip():
                if name is None:
                    raise BuildInputError(f"{path}, line {number}: sequence data before the first '>'")
                parts.append(line.strip())
    if name is not None:
        records.append((name, "".join(parts)))
    return records


def read_reference_tree(path: str):
    """The reference tree and its text; every inner node binary, no label that could be a ghost's."""
    with open(path) as fh:
        text = fh.read().strip()
    try:
        tree = newick.parse(text)
    except newick.NewickError as err:
        raise BuildInputError(f"{path}: {err}") from None
    for i in range(tree.num_nodes):
        if tree.children[i] and len(tree.children[i]) != 2:
            what = f"'{tree.label[i]}'" if tree.label[i] else "an inner node"
            raise BuildInputError(f"{path}: node {i} ({what}) has {len(tree.children[i])} children: the reference tree must be binary "
                                  "and rooted")
        if tree.label[i].startswith(GHOST_PREFIX):
            raise BuildInputError(f"{path}: the label '{tree.label[i]}' of node {i} collides with the ghost nodes' names ({GHOST_PREFIX}*)")
    return tree, text


# ---- extend -------------------------------------------------------------------------------------------------------

def ghost_names(b: int) -> tuple:
    return f"{GHOST_PREFIX}{b}_1", f"{GHOST_PREFIX}{b}_2"


def pendant_lengths(tree: newick.Tree) -> list:
    """Per branch b the mean, over the leaves below b, of the path from the branch's midpoint to the leaf."""
    n = tree.num_nodes
    leaves, below = [0] * n, [0.0] * n   # leaves under a node, and the summed paths from the node down to them
    for i in range(n):                   # post-order: children first
        if not tree.children[i]:
            leaves[i] = 1
        for c in tree.children[i]:
            leaves[i] += leaves[c]
            below[i] += below[c] + leaves[c] * (tree.length[c] or 0.0)
    return [(tree.length[b] or 0.0) / 2.0 + below[b] / leaves[b] for b in range(n)]


def extended_tree(tree: newick.Tree, inner_labels: bool = False) -> newick.Tree:
    """The reference tree with, on every branch b < N - 1, a midpoint M_b and below it P_b with two ghost leaves.
    inner_labels: M_b and P_b named M<b> and P<b>, the reference's inner nodes I<id> (what a reconstruction tool
    does in its own words; tests)."""
    ext = newick.Tree()
    pendant = pendant_lengths(tree)

    def add(children, label, length):
        ext.parent.append(-1)
        ext.children.append(list(children))
        ext.length.append(length)
        ext.label.append(label)
        ext.edge.append(None)
        for c in children:
            ext.parent[c] = ext.num_nodes - 1
        return ext.num_nodes - 1

    top = [0] * tree.num_nodes   # the node of `ext` that stands where b hangs from its parent: M_b
    for b in range(tree.num_nodes):
        kids = [top[c] for c in tree.children[b]]
        label = tree.label[b] if not kids or not inner_labels or tree.label[b] else f"I{b}"
        if b == tree.root:
            top[b] = add(kids, label, tree.length[b])
            continue
        half = (tree.length[b] or 0.0) / 2.0
        node = add(kids, label, half)
        g1, g2 = ghost_names(b)
        p = add([add([], g1, GHOST_LEAF_LENGTH), add([], g2, GHOST_LEAF_LENGTH)], f"P{b}" if inner_labels else "", pendant[b])
        top[b] = add([node, p], f"M{b}" if inner_labels else "", half)
    return ext


def reduce_columns(records: list, reduction: float) -> list:
    """The indices of the columns kept: those whose share of gaps is below `reduction` (1.0 or more: all)."""
    length = len(records[0][1])
    if reduction is None or reduction > 1.0:
        return list(range(length))
    rows = np.array([np.frombuffer(seq.encode(), dtype=np.uint8) for _, seq in records])
    gaps = np.isin(rows, np.frombuffer(GAP_CHARS.encode(), dtype=np.uint8)).mean(axis=0)
    return [int(i) for i in np.flatnonzero(gaps < reduction)]


def checked_alignment(tree_path: str, fasta_path: str, reduction: float | None = None) -> tuple:
    """(tree, its text, the records, the sequence of every name, the indices of the columns kept): the reference tree and its
    alignment read and checked against each other, the columns chosen by --reduction."""
    tree, text = read_reference_tree(tree_path)
    records = read_fasta(fasta_path)
    if not records:
        raise BuildInputError(f"{fasta_path}: no sequences")
    by_name = {}
    for name, seq in records:
        if name in by_name:
            raise BuildInputError(f"{fasta_path}: the sequence '{name}' is given twice")
        if name.startswith(GHOST_PREFIX):
            raise BuildInputError(f"{fasta_path}: the name '{name}' collides with the ghost nodes' names ({GHOST_PREFIX}*)")
        if len(seq) != len(records[0][1]):
            raise BuildInputError(f"{fasta_path}: the sequence '{name}' has {len(seq)} columns, '{records[0][0]}' has "
                                  f"{len(records[0][1])}: the reference must be an alignment")
        by_name[name] = seq
    for leaf in tree.leaves():
        if tree.label[leaf] not in by_name:
            raise BuildInputError(f"{tree_path}: the leaf '{tree.label[leaf]}' has no sequence in {fasta_path}")
    if reduction is not None and not 0.0 < reduction:
        raise BuildInputError("--reduction must be above 0")
    kept = reduce_columns(records, reduction)
    if not kept:
        raise BuildInputError(f"{fasta_path}: --reduction {reduction} removes every column")
    return tree, text, records, by_name, kept


def extend_files(tree_path: str, fasta_path: str, out_dir: str, reduction: float | None = None) -> dict:
    tree, _, records, _, kept = checked_alignment(tree_path, fasta_path, reduction)
    os.makedirs(out_dir, exist_ok=True)
    paths = {name: os.path.join(out_dir, name) for name in ("extended.nwk", "extended.fasta", "columns.tsv")}
    with open(paths["extended.nwk"], "w") as fh:
        fh.write(newick.write(extended_tree(tree)) + "\n")
    index = np.array(kept, dtype=np.int64)
    with open(paths["extended.fasta"], "w") as fh:
        for name, seq in records:
            row = np.frombuffer(seq.encode(), dtype=np.uint8)[index].tobytes().decode()
            fh.write(f">{name}\n{row}\n")
        for b in range(tree.num_nodes - 1):
            for name in ghost_names(b):
                fh.write(f">{name}\n{'-' * len(kept)}\n")
    with open(paths["columns.tsv"], "w") as fh:
        fh.write("column\toriginal\n")
        for new, old in enumerate(kept):
            fh.write(f"{new}\t{old}\n")
    return paths


# ---- the ghost nodes of a tree written back ---------------------------------------------------------------------------

def ghost_node_labels(tree: newick.Tree, ar_tree: newick.Tree, what: str = "the --ar-tree") -> list:
    """Per branch b < N - 1 of the reference `tree` the labels (M_b, P_b) that the reconstruction gave the midpoint
    and the pendant node, found by adjacency in `ar_tree` however it is rooted; the whole topology is checked to be the
    extension of `tree`."""
    near = ar_tree.neighbours()
    leaf_of = {}
    for i in range(ar_tree.num_nodes):
        if len(near[i]) == 1 and ar_tree.label[i]:
            leaf_of[ar_tree.label[i]] = i
    n = tree.num_nodes
    m_of, p_of = [None] * n, [None] * n
    for b in range(n - 1):
        hosts = []
        for name in ghost_names(b):
            if name not in leaf_of:
                raise BuildInputError(f"{what} has no leaf '{name}': branch {b} has no ghost nodes")
            hosts.append(near[leaf_of[name]][0])
        if hosts[0] != hosts[1]:
            raise BuildInputError(f"{what}: the ghost leaves of branch {b} do not hang from one node")
        p = hosts[0]
        rest = [x for x in near[p] if x not in (leaf_of[ghost_names(b)[0]], leaf_of[ghost_names(b)[1]])]
        if len(rest) != 1:
            raise BuildInputError(f"{what}: the pendant node of branch {b} has {len(near[p])} neighbours, not 3")
        m_of[b], p_of[b] = rest[0], p
    # the topology: M_b lies between b's node and its parent's
    for b in range(n - 1):
        others = [x for x in near[m_of[b]] if x != p_of[b]]
        wrong = BuildInputError(f"{what} is not the extension of the reference tree at branch {b}")
        if len(others) != 2:
            raise wrong
        if tree.is_leaf(b):
            if leaf_of.get(tree.label[b]) not in others:
                raise wrong
        else:
            want = {m_of[b]} | {m_of[c] for c in tree.children[b]}
            if not any(set(near[x]) == want for x in others):
                raise wrong
        parent = tree.parent[b]
        if parent == tree.root:
            sibling = [c for c in tree.children[parent] if c != b][0]
            if m_of[sibling] not in others and not any(set(near[x]) == {m_of[b], m_of[sibling]} for x in others):
                raise wrong
    labels = []
    for b in range(n - 1):
        m, p = ar_tree.label[m_of[b]], ar_tree.label[p_of[b]]
        if not m or not p:
            raise BuildInputError(f"{what}: the {'midpoint' if not m else 'pendant'} node of branch {b} has no label")
        labels.append((m, p))
    return labels


# ---- the posterior file -----------------------------------------------------------------------------------------------

def read_ar_header(line: str, states: str, path: str) -> tuple:
    """(column of Node, column of Site, the column of every state in alphabet order) from the header line."""
    names = [c.strip() for c in line.rstrip("\r\n").split("\t")]
    lower = [c.lower() for c in names]
    for needed in ("node", "site"):
        if needed not in lower:
            raise BuildInputError(f"{path}, line 1: the header has no '{needed.capitalize()}' column")
    columns = []
    for state in alphabet.state_chars(states):
        want = f"p_{state.lower()}"
        if want not in lower:
            raise BuildInputError(f"{path}, line 1: the header has no column 'p_{state}' for state {state}")
        columns.append(lower.index(want))
    return lower.index("node"), lower.index("site"), columns


def ghost_posteriors(fh, states: str, wanted, path: str = "the posterior file"):
    """Streams a posterior table: yields (node label, float32 [L][sigma]) for every node of `wanted`, in file order, once
    its rows have ended; rows of other nodes are skipped.  Every node must have the sites 1 .. L once each, L the first
    yielded node's."""
    header = fh.readline()
    if not header.strip():
        raise BuildInputError(f"{path}: empty")
    node_col, site_col, state_cols = read_ar_header(header, states, path)
    need = max([node_col, site_col] + state_cols)
    sigma = len(state_cols)
    current, rows, seen_sites, done = None, [], set(), set()
    first_line = last_line = 0
    length = [None]

    def close():
        sites = len(rows)
        missing = next((s for s in range(1, max(seen_sites) + 1) if s not in seen_sites), None)
        if missing is not None:
            raise BuildInputError(f"{path}, line {last_line}: node '{current}' (from line {first_line}) ends with site {missing} missing")
        if length[0] is None:
            length[0] = sites
        if sites != length[0]:
            raise BuildInputError(f"{path}, line {last_line}: node '{current}' (from line {first_line}) has {sites} sites, the ghost "
                                  f"nodes before it have {length[0]}")
        out = np.zeros((sites, sigma), dtype=np.float32)
        for site, probs in rows:
            out[site - 1] = probs
        return current, out

    for number, line in enumerate(fh, 2):
        if not line.strip():
            continue
        fields = line.rstrip("\r\n").split("\t")
        if len(fields) <= need:
            raise BuildInputError(f"{path}, line {number}: {len(fields)} fields, the header has more")
        node = fields[node_col].strip()
        if node != current:
            if current is not None and current in wanted:
                yield close()
                done.add(current)
            current, rows, seen_sites, first_line = node, [], set(), number
            if node in done:
                raise BuildInputError(f"{path}, line {number}: the rows of node '{node}' are not together: its sites would repeat")
        if node not in wanted:
            continue
        last_line = number
        try:
            site = int(fields[site_col])
        except ValueError:
            raise BuildInputError(f"{path}, line {number}: '{fields[site_col]}' is no site number") from None
        if site < 1:
            raise BuildInputError(f"{path}, line {number}: site {site} (sites are 1-based)")
        if site in seen_sites:
            raise BuildInputError(f"{path}, line {number}: site {site} of node '{node}' is given twice")
        probs = []
        for col in state_cols:
            try:
                p = float(fields[col])
            except ValueError:
                raise BuildInputError(f"{path}, line {number}: '{fields[col]}' is no number") from None
            if not 0.0 <= p <= 1.0:
                raise BuildInputError(f"{path}, line {number}: the probability {fields[col]} lies outside [0, 1]")
            probs.append(p)
        seen_sites.add(site)
        rows.append((site, probs))
    if current is not None and current in wanted:
        yield close()


# ---- build --------------------------------------------------------------------------------------------------------

GHOST_CHOICES = ("inner", "outer", "both")


def check_build_options(states: str, kmer_size: int, omega: float, chunk: int) -> None:
    """What can be refused before a file is opened."""
    sigma = alphabet.alphabet_size(states)
    top = 15 if sigma == 4 else 7
    if not 2 <= int(kmer_size) <= top:
        raise BuildInputError(f"-k must lie in [2, {top}] for -s {states}, not {kmer_size}")
    if not 0.0 < float(omega) <= float(sigma):
        raise BuildInputError(f"--omega must lie in (0, {sigma}] for -s {states} (the threshold (omega / {sigma})^k is a probability), "
                              f"not {omega}")
    if int(chunk) < 1:
        raise BuildInputError(f"--chunk must be at least 1, not {chunk}")


def check_filter_options(filter: str, filter_seed) -> None:
    """--filter and --filter-seed: what can be refused before a file is opened."""
    from . import filters
    if filter not in filters.FILTERS:
        raise BuildInputError(f"--filter: '{filter}' is no filter (one of {', '.join(filters.FILTERS)})")
    if filter_seed is not None and filter != "random":
        raise BuildInputError("--filter-seed needs --filter random")
    if filter_seed is not None and not 0 <= int(filter_seed) < 2 ** 64:
        raise BuildInputError(f"--filter-seed must be a uint64, not {filter_seed}")


def ranked_order(db, filter: str, filter_seed, host: bool = False, num_threads: int = 1, device: int = 0):
    """The order dbfile.write_db is given for `filter`: None for "best" (its own, unchanged), else the ranking's."""
    from . import filters
    if filter == "best":
        return None
    return filters.rank_db(db, filter, filter_seed or 0, host=host, num_threads=num_threads, device=device)[1]


def rerank_file(in_path: str, out_path: str, filter: str, filter_seed=None, host: bool = False, num_threads: int = 1,
                device: int = 0) -> dict:
    """`epik.py rank`: a database file read whole (mu = 1, its own omega), ranked by `filter`, written to out_path."""
    import struct

    from . import dbfile, filters
    check_filter_options(filter, filter_seed)
    try:
        with open(in_path, "rb") as fh:
            head = fh.read(24)
        if len(head) < 24 or head[:8] != dbfile.MAGIC:
            raise RuntimeError(f"{in_path} is not an EPIKAMD1 file")
        built_omega = struct.unpack("<f", head[20:24])[0]
        dense, text = dbfile.read_db(in_path, mu=1.0, omega=built_omega)
    except (RuntimeError, OSError, struct.error) as err:
        raise BuildInputError(str(err)) from None
    lens = np.diff(dense.offsets.astype(np.int64))
    keys = np.flatnonzero(lens)
    offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens[keys])
    db = dense
    db.keys, db.offsets = keys.astype(np.uint32), offsets      # the sparse form of the same lists: values stay as they lie
    db.omega = built_omega                                     # (the header's own float32, written back bit for bit)
    order = filters.rank_db(db, filter, filter_seed or 0, host=host, num_threads=num_threads, device=device)[1]
    dbfile.write_db(out_path, db, text, order=order)
    return dict(num_keys=len(keys), num_entries=int(db.values.shape[0]), num_branches=db.num_branches)


def build_from_files(tree_path: str, ar_probs: str, ar_tree: str, states: str, kmer_size: int, omega: float, out_path: str,
                     ghosts: str = "both", chunk: int = 256, device: int = 0, workspace_bytes: int = 0, host: bool = False,
                     filter: str = "best", filter_seed: int | None = None) -> dict:
    """`epik.py build`.  host=True runs the host mirror over all ghost nodes at once instead of the device builder
    (no GPU: tests of the file side).  `filter` ranks the k-mers of the file (epik_amd/filters.py); "best" is the order
    dbfile.write_db has always written."""
    from . import build, dbfile
    check_build_options(states, kmer_size, omega, chunk)
    check_filter_options(filter, filter_seed)
    if ghosts not in GHOST_CHOICES:
        raise BuildInputError(f"--ghosts must be one of {', '.join(GHOST_CHOICES)}, not '{ghosts}'")
    tree, text = read_reference_tree(tree_path)
    with open(ar_tree) as fh:
        try:
            written_back = newick.parse(fh.read().strip())
        except newick.NewickError as err:
            raise BuildInputError(f"{ar_tree}: {err}") from None
    labels = ghost_node_labels(tree, written_back, what=ar_tree)
    wanted = {}
    for b, (m, p) in enumerate(labels):
        for label, chosen in ((m, ghosts in ("inner", "both")), (p, ghosts in ("outer", "both"))):
            if chosen:
                if label in wanted:
                    raise BuildInputError(f"{ar_tree}: the label '{label}' names two ghost nodes (branches {wanted[label]} and {b})")
                wanted[label] = b
    n = tree.num_nodes
    found = set()
    batch_p, batch_b = [], []
    chunks = []

    def flush(builder):
        if not batch_p:
            return
        logp = build.logp_from_posteriors(np.stack(batch_p))
        branch_of = np.array(batch_b, dtype=np.uint32)
        if builder is None:
            chunks.append((logp, branch_of))
        else:
            builder.add(logp, branch_of)
        batch_p.clear(), batch_b.clear()

    def stream(builder):
        with open(ar_probs) as fh:
            for label, probs in ghost_posteriors(fh, states, wanted, path=ar_probs):
                if probs.shape[0] < kmer_size:
                    raise BuildInputError(f"{ar_probs}: node '{label}' has {probs.shape[0]} sites, fewer than k = {kmer_size}")
                found.add(label)
                batch_p.append(probs)
                batch_b.append(wanted[label])
                if len(batch_p) >= chunk:
                    flush(builder)
            flush(builder)
        for label, b in wanted.items():
            if label not in found:
                raise BuildInputError(f"{ar_probs}: no rows for node '{label}', a ghost node of branch {b}")

    if host:
        stream(None)
        sigma = alphabet.alphabet_size(states)
        logp = np.concatenate([c[0] for c in chunks]) if chunks else np.zeros((0, kmer_size, sigma), np.float32)
        branch_of = np.concatenate([c[1] for c in chunks]) if chunks else np.zeros(0, np.uint32)
        db = build.build_host(states, kmer_size, n, logp, branch_of, omega=omega)
        order = ranked_order(db, filter, filter_seed, host=True)
    else:
        with build.Builder(states, kmer_size, n, omega=omega, device=device, workspace_bytes=workspace_bytes) as builder:
            stream(builder)
            db = builder.finish()
            order = None if filter == "best" else builder.rank(filter, filter_seed or 0)[1]
    dbfile.write_db(out_path, db, text, order=order)
    return dict(num_keys=int(db.keys.shape[0]), num_entries=db.num_entries, ghost_nodes=len(wanted), num_branches=n)


# ---- reconstruct ------------------------------------------------------------------------------------------------------

def write_ar_files(probs_path: str, tree_out_path: str, tree: newick.Tree, states: str, post, branch_of, ghosts: str) -> None:
    """The posteriors in the layout `build` reads (read_ar_header / ghost_posteriors): nodes M<b> and P<b>, 1-based sites,
    %.9g (a float32 read back is the same float32), and the extended tree with those labels."""
    with open(tree_out_path, "w") as fh:
        fh.write(newick.write(extended_tree(tree, inner_labels=True)) + "\n")
    outer_from = tree.num_nodes - 1 if ghosts == "both" else (0 if ghosts == "outer" else post.shape[0])
    with open(probs_path, "w") as fh:
        fh.write("Node\tSite\tState\t" + "\t".join(f"p_{c}" for c in alphabet.state_chars(states)) + "\n")
        letters = np.array(list(alphabet.state_chars(states)))
        for g in range(post.shape[0]):
            label = f"{'P' if g >= outer_from else 'M'}{int(branch_of[g])}"
            best = letters[post[g].argmax(axis=1)]
            for site in range(post.shape[1]):
                fh.write(f"{label}\t{site + 1}\t{best[site]}\t" + "\t".join("%.9g" % v for v in post[g, site]) + "\n")


def build_from_alignment(tree_path: str, fasta_path: str, model: str, states: str, kmer_size: int, omega: float, out_path: str,
                         model_file: str | None = None, ghosts: str = "both", reduction: float | None = None, chunk: int = 256,
                         device: int = 0, workspace_bytes: int = 0, host: bool = False, num_threads: int = 1,
                         write_ar_probs: str | None = None, write_ar_tree: str | None = None, filter: str = "best",
                         filter_seed: int | None = None) -> dict:
    """`epik.py reconstruct`: tree and alignment to a database, the ancestral posteriors computed here.  host=True runs
    the host mirrors of the reconstruction, of the builder and of the ranking (no GPU)."""
    from . import ancestral, build, dbfile
    check_build_options(states, kmer_size, omega, chunk)
    check_filter_options(filter, filter_seed)
    if ghosts not in GHOST_CHOICES:
        raise BuildInputError(f"--ghosts must be one of {', '.join(GHOST_CHOICES)}, not '{ghosts}'")
    if bool(write_ar_probs) != bool(write_ar_tree):
        raise BuildInputError("--write-ar-probs and --write-ar-tree go together: `build` reads both")
    try:
        parsed = ancestral.Model.parse(model, states)   # (before anything is opened)
        parsed.check_model_file(model_file)
    except ancestral.ModelError as err:
        raise BuildInputError(f"--model: {err}") from None
    tree, text, _, by_name, kept = checked_alignment(tree_path, fasta_path, reduction)
    if len(kept) < kmer_size:
        raise BuildInputError(f"{fasta_path}: {len(kept)} columns are kept, fewer than k = {kmer_size}")
    if tree.num_nodes < 3:
        raise BuildInputError(f"{tree_path}: a reference tree has at least two leaves")
    masks = ancestral.leaf_masks(tree, by_name, states, kept)
    try:
        parsed.resolve(model_file, masks)
        weights, p_full, p_half, p_pend = parsed.tables(tree)
    except ancestral.ModelError as err:
        raise BuildInputError(f"--model: {err}") from None
    except OSError as err:
        raise BuildInputError(f"--model-file: {err}") from None
    inputs = (ancestral.tree_parent(tree), parsed.sigma, weights, parsed.freqs, p_full, p_half, p_pend)
    if host:
        post, branch_of, dead = ancestral.posteriors_host(*inputs, masks, ghosts, num_threads=num_threads)
    else:
        with ancestral.Ancestral(*inputs, device=device, workspace_bytes=workspace_bytes) as handle:
            post, branch_of, dead = handle.posteriors(masks, ghosts)
    if write_ar_probs:
        write_ar_files(write_ar_probs, write_ar_tree, tree, states, post, branch_of, ghosts)
    n = tree.num_nodes
    if host:
        db = build.build_host(states, kmer_size, n, build.logp_from_posteriors(post), branch_of, omega=omega, num_threads=num_threads)
        order = ranked_order(db, filter, filter_seed, host=True, num_threads=num_threads)
    else:
        with build.Builder(states, kmer_size, n, omega=omega, device=device) as builder:
            for g in range(0, post.shape[0], chunk):
                builder.add(build.logp_from_posteriors(post[g:g + chunk]), branch_of[g:g + chunk])
            db = builder.finish()
            order = None if filter == "best" else builder.rank(filter, filter_seed or 0)[1]
    dbfile.write_db(out_path, db, text, order=order)
    return dict(num_keys=int(db.keys.shape[0]), num_entries=db.num_entries, ghost_nodes=int(post.shape[0]), num_branches=n,
                sites=int(post.shape[1]), dead_sites=int(dead), categories=parsed.num_categories)
