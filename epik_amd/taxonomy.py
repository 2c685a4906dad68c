"""Taxonomic assignment (include/epik_amd.h: epik_amd_taxonomy): the taxonomy file, the numbering of its taxa and the
labels of the branches as epik_amd/host/taxonomy.cpp reads, numbers and gives them; the rule of the records and the
cells over whole arrays (`numpy_assign`), worded after the header; the device object (`DeviceTaxonomy`) and the rule on
the host through the library (`assign_host`)."""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import capi

LWR_BITS = capi.PROFILE_LWR_BITS
TOO_NARROW = capi.ROWS_COUNTS_TOO_NARROW
U64 = np.uint64
TOTALS = ("placed", "no_hit", "too_short", "too_narrow", "no_mass", "bad_reads")


class TaxonomyError(ValueError):
    """A taxonomy file, or a tree it does not fit: the message names the line, the leaf or the branch."""


def mass_tau_q(share: float) -> int:
    """--taxonomy-mass as the rule takes it: llrint(share * 2^30), share in (0.5, 1]; the result lies in (2^29, 2^30]."""
    share = float(share)
    tq = int(np.rint(np.float64(share) * np.float64(1 << LWR_BITS))) if 0.0 <= share <= 1.0 else 0
    if not (1 << (LWR_BITS - 1)) < tq <= (1 << LWR_BITS):
        raise ValueError(f"the taxonomy mass must lie in (0.5, 1], not {share}")
    return tq


@dataclass
class Taxonomy:
    """The taxa of a taxonomy file: post-order ids over the trie of the taxopaths, children in bytewise order."""

    parent: np.ndarray                  # int64 [T], -1 for the root (T - 1)
    first: np.ndarray                   # int64 [T]: the clade of t is [first[t], t]
    path: list                          # [T] taxopaths, ";"-joined; "" for the root
    leaf: list = field(default_factory=list)        # the leaf labels of the file, in file order
    leaf_taxon: list = field(default_factory=list)  # ... their taxa
    leaf_line: list = field(default_factory=list)   # ... and their lines (from 1)

    @property
    def num_taxa(self) -> int:
        return len(self.parent)

    def parents(self) -> np.ndarray:
        """taxon_parent[] as the C ABI takes it."""
        return np.where(self.parent < 0, capi.TREE_NO_PARENT, self.parent).astype(np.uint32)


_BLANKS = " \t\r\n\v\f"


def parse_taxonomy(text) -> Taxonomy:
    """`text`: the file's content (str or bytes)."""
    if isinstance(text, bytes):
        text = text.decode("utf-8", errors="surrogateescape")
    children, parent_of, name_of = [{}], [-1], [""]
    leaf, leaf_node, leaf_line, seen = [], [], [], {}
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for number, line in enumerate(lines, 1):
        at = f"line {number}: "
        if not line.strip(_BLANKS) or line.strip(_BLANKS)[0] == "#":
            continue
        if "\t" not in line:
            raise TaxonomyError(at + "no tab between the leaf label and the taxopath")
        label, whole = line.split("\t", 1)
        label, whole = label.strip(_BLANKS), whole.strip(_BLANKS)
        if not label:
            raise TaxonomyError(at + "an empty leaf label")
        if label in seen:
            raise TaxonomyError(at + f"leaf {label} is given twice (first on line {seen[label]})")
        seen[label] = number
        node = 0
        if whole != "-":
            for name in whole.split(";"):
                name = name.strip(_BLANKS)
                if not name:
                    raise TaxonomyError(at + f"an empty element in the taxopath of leaf {label}")
                if name not in children[node]:
                    children[node][name] = len(children)
                    children.append({})
                    parent_of.append(node)
                    name_of.append(name)
                node = children[node][name]
        leaf.append(label), leaf_node.append(node), leaf_line.append(number)
    total = len(children)
    key = (lambda s: s.encode("utf-8", errors="surrogateescape"))
    ordered = [[children[v][k] for k in sorted(children[v], key=key)] for v in range(total)]
    ids, first_of, nxt = [0] * total, [0] * total, 0
    stack = [(0, 0)]
    while stack:
        node, at_child = stack.pop()
        if at_child < len(ordered[node]):
            stack.append((node, at_child + 1))
            child = ordered[node][at_child]
            first_of[child] = nxt
            stack.append((child, 0))
            continue
        ids[node] = nxt
        nxt += 1
    parent, first, path = np.full(total, -1, np.int64), np.zeros(total, np.int64), [""] * total
    node_of = [0] * total
    for node in range(total):
        node_of[ids[node]] = node
        first[ids[node]] = first_of[node]
        if node:
            parent[ids[node]] = ids[parent_of[node]]
    for t in range(total - 2, -1, -1):
        above = path[parent[t]]
        path[t] = name_of[node_of[t]] if not above else above + ";" + name_of[node_of[t]]
    return Taxonomy(parent, first, path, leaf, [ids[v] for v in leaf_node], leaf_line)


def label_branches(taxa: Taxonomy, tree_parent, names) -> np.ndarray:
    """label[N] (uint32) for the tree `tree_parent` (post-order ids; the root's parent -1 or capi.TREE_NO_PARENT) whose
    leaves -- the branches without children -- are named names[b]."""
    tree_parent = np.asarray(tree_parent).astype(np.int64)
    n = len(tree_parent)
    tree_parent = np.where((tree_parent < 0) | (tree_parent >= n), -1, tree_parent)
    depth = np.zeros(taxa.num_taxa, np.int64)
    for t in range(taxa.num_taxa - 2, -1, -1):
        depth[t] = depth[taxa.parent[t]] + 1

    def common(a, b):
        while depth[a] > depth[b]:
            a = int(taxa.parent[a])
        while depth[b] > depth[a]:
            b = int(taxa.parent[b])
        while a != b:
            a, b = int(taxa.parent[a]), int(taxa.parent[b])
        return a

    inner = np.zeros(n, bool)
    inner[tree_parent[:-1][tree_parent[:-1] >= 0]] = True
    entry = {name: k for k, name in enumerate(taxa.leaf)}
    used = [False] * len(taxa.leaf)
    label = [-1] * n
    for b in range(n):
        if inner[b]:
            continue
        if names[b] not in entry:
            raise TaxonomyError(f"leaf {names[b]}: the taxonomy file does not give it")
        used[entry[names[b]]] = True
        label[b] = taxa.leaf_taxon[entry[names[b]]]
    for k, was in enumerate(used):
        if not was:
            raise TaxonomyError(f"line {taxa.leaf_line[k]}: {taxa.leaf[k]} is no leaf of the tree")
    for b in range(n - 1):
        p = int(tree_parent[b])
        label[p] = label[b] if label[p] < 0 else common(label[p], label[b])
    return np.array(label, dtype=np.uint32)


def groups_at_rank(taxa: Taxonomy, label, depth: int):
    """The groups painting by windows calls (epik_amd/windows.py), cut at `depth` >= 1 elements of the taxopath: the
    group of a branch is the depth-`depth` ancestor of its label when the label is at least that deep, else
    capi.WINDOW_NO_GROUP; group ids number the taxa of that depth in ascending taxon id.  Returns (group uint32 [N],
    the taxon of every group)."""
    depth = int(depth)
    if depth < 1:
        raise ValueError(f"the window rank must be at least 1, not {depth}")
    T = taxa.num_taxa
    deep = np.zeros(T, np.int64)
    for t in range(T - 2, -1, -1):
        deep[t] = deep[taxa.parent[t]] + 1
    anc = np.arange(T)                    # the ancestor of t at `depth`, for the taxa at least that deep
    for t in range(T - 2, -1, -1):
        if deep[t] > depth:
            anc[t] = anc[taxa.parent[t]]
    group_taxa = np.flatnonzero(deep == depth)
    id_of = np.full(T, capi.WINDOW_NO_GROUP, np.int64)
    id_of[group_taxa] = np.arange(len(group_taxa))
    label = np.asarray(label).astype(np.int64)
    group = np.where(deep[label] >= depth, id_of[anc[label]], capi.WINDOW_NO_GROUP)
    return group.astype(np.uint32), [int(t) for t in group_taxa]


def taxonomy_first(parent) -> np.ndarray:
    """first[] of parent[] (-1 or capi.TREE_NO_PARENT for the root), by subtree sizes."""
    parent = np.asarray(parent).astype(np.int64)
    size = np.ones(len(parent), np.int64)
    for t in range(len(parent) - 1):
        size[parent[t]] += size[t]
    return np.arange(len(parent)) - size + 1


def _walk_lca(parent, first, a, b):
    """lca of many pairs at once by steps up parent[]: every pair steps until its node's clade holds both."""
    lo, c = np.minimum(first[a], first[b]), np.maximum(a, b)
    while True:
        up = first[c] > lo
        if not up.any():
            return c
        c[up] = parent[c[up]]


@dataclass
class TaxaCells:
    """What the rule adds: `direct` and `assigned` uint64 [S][T], `totals` a record array [S] (capi.TAXA_TOTALS) and
    `bad_samples`."""

    direct: np.ndarray
    assigned: np.ndarray
    totals: np.ndarray
    bad_samples: int = 0

    def same_as(self, other) -> bool:
        return (np.array_equal(self.direct, other.direct) and np.array_equal(self.assigned, other.assigned)
                and np.array_equal(self.totals, other.totals) and self.bad_samples == other.bad_samples)


def clade_sums(cells, first) -> np.ndarray:
    """clade[..., t] = the sum of cells[..., first[t] .. t], wrapping: differences of one prefix sum."""
    cells = np.asarray(cells, dtype=U64)
    prefix = np.concatenate([np.zeros(cells.shape[:-1] + (1,), U64), np.cumsum(cells, axis=-1, dtype=U64)], axis=-1)
    first = np.asarray(first).astype(np.int64)
    return prefix[..., 1:] - prefix[..., first]


def numpy_records(taxon_parent, label, rows, n_rows, counts, tau_q):
    """The records of the rule of include/epik_amd.h over a batch, as capi.TAXON_RECORD [n], and what `numpy_cells`
    needs of them.  The candidates of a read's taxon are its rows' taxa and the lcas of the id-sorted neighbours among
    them; every comparison is made on Python ints."""
    parent = np.asarray(taxon_parent).astype(np.int64)
    T = len(parent)
    parent = np.where((parent < 0) | (parent >= T), T - 1, parent)   # (the root steps onto itself)
    first = taxonomy_first(np.where(np.arange(T) == T - 1, -1, parent))
    label = np.asarray(label).astype(np.int64)
    N = len(label)
    n, keep = rows.shape
    tau_q = int(tau_q)
    assert (1 << (LWR_BITS - 1)) < tau_q <= (1 << LWR_BITS)
    n_rows = np.asarray(n_rows).astype(np.int64)
    cls = np.zeros(n, np.int64)
    cls[n_rows == TOO_NARROW] = capi.TAXON_TOO_NARROW
    cls[(cls == 0) & (n_rows == 0)] = capi.TAXON_TOO_SHORT
    cls[(cls == 0) & (np.asarray(counts)[:, 0] == 0)] = capi.TAXON_NO_HIT
    live = np.where(cls != 0, 0, np.minimum(n_rows, keep))
    slot = np.arange(keep)[None, :] < live[:, None]
    branch = rows["branch"].astype(np.int64)
    cls[(slot & (branch >= N)).any(axis=1)] = capi.TAXON_BAD_ROW
    mine = slot & (cls == 0)[:, None]
    t = np.where(mine, label[np.where(mine, branch, 0)], T)            # T: no taxon (sorts behind all)
    q = np.rint(np.where(mine, rows["lwr"], 0.0) * np.float64(1 << LWR_BITS)).astype(np.int64).astype(U64)
    total = q.sum(axis=1, dtype=U64)
    cls[(cls == 0) & (total == 0)] = capi.TAXON_NO_MASS
    placed = cls == 0
    mine &= placed[:, None]
    t = np.where(mine, t, T)

    ts = np.sort(t, axis=1)
    cand = np.full((n, max(2 * keep - 1, 1)), T, np.int64)
    cand[:, :keep] = ts
    if keep > 1:
        a, b = ts[:, :-1], ts[:, 1:]
        both = b < T
        adj = np.full(a.shape, T, np.int64)
        adj[both] = _walk_lca(parent, first, a[both], b[both])
        cand[:, keep:] = adj
    first_ext, best, best_mass = np.append(first, T + 1), np.full(n, T, np.int64), np.zeros(n, U64)
    for lo in range(0, n, 256):
        sl = slice(lo, min(lo + 256, n))
        c = cand[sl]
        inside = (first_ext[c][:, :, None] <= t[sl][:, None, :]) & (t[sl][:, None, :] <= c[:, :, None])
        mass = (inside * q[sl][:, None, :]).sum(axis=2, dtype=U64)
        at = np.nonzero((mass > 0) & placed[sl][:, None])
        need = total[sl][at[0]].astype(object) * tau_q
        ok = np.zeros(mass.shape, bool)
        ok[at] = [(int(m) << LWR_BITS) >= r for m, r in zip(mass[at], need)]
        lowest = np.where(ok, c, T)
        pick = lowest.argmin(axis=1)
        best[sl] = lowest[np.arange(len(pick)), pick]
        best_mass[sl] = mass[np.arange(len(pick)), pick]
    assert (best[placed] < T).all()

    records = np.zeros(n, dtype=capi.TAXON_RECORD)
    records["taxon"] = np.where(placed, best, cls)
    records["taxon_mass_q"] = np.where(placed, np.minimum(best_mass, U64(0xFFFFFFFF)), 0)
    records["first_taxon"] = np.where(placed, t[:, 0], 0)
    records["total_q"] = np.where(placed, np.minimum(total, U64(0xFFFFFFFF)), 0)
    return records, dict(T=T, cls=cls, placed=placed, mine=mine, t=t, q=q, best=best)


def numpy_cells(state, weights=None, samples=None, num_samples=1) -> TaxaCells:
    """The cells the reads of `numpy_records` add, read i with weights[i] (None: 1) into row samples[i] (None: 0)."""
    T, cls, placed, mine, t, q, best = (state[k] for k in ("T", "cls", "placed", "mine", "t", "q", "best"))
    n = len(cls)
    S = int(num_samples)
    smp = np.zeros(n, np.int64) if samples is None else np.asarray(samples).astype(np.int64)
    w = np.ones(n, U64) if weights is None else np.asarray(weights).astype(U64)
    known = smp < S
    cells = TaxaCells(np.zeros((S, T), U64), np.zeros((S, T), U64), np.zeros(S, dtype=capi.TAXA_TOTALS), int((~known).sum()))
    sel = known & placed
    np.add.at(cells.assigned, (smp[sel], best[sel]), w[sel])
    rows_sel = mine & sel[:, None]
    smp_rows, w_rows = np.broadcast_to(smp[:, None], mine.shape), np.broadcast_to(w[:, None], mine.shape)
    np.add.at(cells.direct, (smp_rows[rows_sel], t[rows_sel]), w_rows[rows_sel] * q[rows_sel])
    for name, code in (("placed", 0), ("no_hit", capi.TAXON_NO_HIT), ("too_short", capi.TAXON_TOO_SHORT),
                       ("too_narrow", capi.TAXON_TOO_NARROW), ("no_mass", capi.TAXON_NO_MASS), ("bad_reads", capi.TAXON_BAD_ROW)):
        which = known & (cls == code)
        np.add.at(cells.totals[name], smp[which], U64(1) if name == "bad_reads" else w[which])
    return cells


def numpy_assign(taxon_parent, label, rows, n_rows, counts, tau_q, weights=None, samples=None, num_samples=1):
    """(records, TaxaCells) of a batch: `numpy_records`, then `numpy_cells`."""
    records, state = numpy_records(taxon_parent, label, rows, n_rows, counts, tau_q)
    return records, numpy_cells(state, weights, samples, num_samples)


def _u32(a, n=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if n is not None and a.shape != (n,):
        raise ValueError(f"expected {n} values, not {a.shape}")
    return a


def assign_host(taxon_parent, label, rows, n_rows, counts, tau_q, weights=None, samples=None, num_samples=1,
                want_records=True, want_cells=True):
    """The rule on the host through the library (`epik_amd_taxonomy_assign_host`): (records or None, TaxaCells or None)."""
    lib = capi.load()
    parent = np.asarray(taxon_parent).astype(np.int64)
    parent = np.ascontiguousarray(np.where(parent < 0, capi.TREE_NO_PARENT, parent).astype(np.uint32))
    label = _u32(label)
    rows = np.ascontiguousarray(rows, dtype=capi.PLACEMENT)
    n, keep = rows.shape
    n_rows, counts = _u32(n_rows, n), np.ascontiguousarray(counts, dtype=np.uint32)
    weights, samples = _u32(weights, n), _u32(samples, n)
    T, S = len(parent), int(num_samples)
    records = np.zeros(n, dtype=capi.TAXON_RECORD) if want_records else None
    cells = TaxaCells(np.zeros((S, T), U64), np.zeros((S, T), U64), np.zeros(S, dtype=capi.TAXA_TOTALS)) if want_cells else None
    bad = ctypes.c_uint64(0)
    ptr = (lambda a: None if a is None else a.ctypes.data)
    capi.check(lib.epik_amd_taxonomy_assign_host(
        parent.ctypes.data, T, label.ctypes.data, len(label), keep, rows.ctypes.data, n_rows.ctypes.data, counts.ctypes.data,
        ptr(weights), ptr(samples), n, S, int(tau_q), ptr(records),
        cells.direct.ctypes.data if cells else None, cells.assigned.ctypes.data if cells else None,
        cells.totals.ctypes.data if cells else None, ctypes.byref(bad) if cells else None))
    if cells:
        cells.bad_samples = int(bad.value)
    return records, cells


class DeviceTaxonomy:
    """A device taxonomy object of `num_samples` samples for one placer (`epik_amd_taxonomy_create`): all zero at first.
    A context manager; `close()` frees it."""

    def __init__(self, placer, taxon_parent, label, num_samples: int = 1):
        self._lib = capi.load()
        self._handle = ctypes.c_void_p()
        parent = np.asarray(taxon_parent).astype(np.int64)
        parent = np.ascontiguousarray(np.where(parent < 0, capi.TREE_NO_PARENT, parent).astype(np.uint32))
        label = _u32(label)
        if len(label) != placer.num_branches:
            raise ValueError(f"label holds {len(label)} branches, the placer has {placer.num_branches}")
        capi.check(self._lib.epik_amd_taxonomy_create(placer._handle, parent.ctypes.data, len(parent), label.ctypes.data,
                                                      int(num_samples), ctypes.byref(self._handle)))
        self.device = placer.device
        self.num_taxa, self.num_samples = len(parent), int(num_samples)
        self.num_branches, self.keep_at_most = placer.num_branches, placer.keep_at_most

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.epik_amd_taxonomy_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def lds_path(self) -> bool:
        """Whether add_device sums the current sample in LDS first (else straight into global memory)."""
        lds = ctypes.c_uint32(0)
        capi.check(self._lib.epik_amd_taxonomy_info(self._handle, None, None, None, ctypes.byref(lds)))
        return bool(lds.value)

    def reset(self) -> None:
        capi.check(self._lib.epik_amd_taxonomy_reset(self._handle))

    def add_device(self, d_rows: int, d_n_rows: int, d_kmer_counts: int, n: int, tau_q: int, d_records: int = 0,
                   d_weights: int = 0, d_samples: int = 0, stream: int = 0) -> None:
        """Device pointers, asynchronous on `stream` (`epik_amd_taxonomy_add_device`); `d_records` 0: cells only."""
        capi.check(self._lib.epik_amd_taxonomy_add_device(self._handle, d_rows or None, d_n_rows or None, d_kmer_counts or None,
                                                          d_weights or None, d_samples or None, int(n), int(tau_q),
                                                          d_records or None, stream or None))

    def read(self) -> TaxaCells:
        """Synchronises the device and returns the cells (`epik_amd_taxonomy_read`)."""
        shape = (self.num_samples, self.num_taxa)
        cells = TaxaCells(np.zeros(shape, U64), np.zeros(shape, U64), np.zeros(self.num_samples, dtype=capi.TAXA_TOTALS))
        bad = ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_taxonomy_read(self._handle, cells.direct.ctypes.data, cells.assigned.ctypes.data,
                                                    cells.totals.ctypes.data, ctypes.byref(bad)))
        cells.bad_samples = int(bad.value)
        return cells

    def add_cells(self, cells: TaxaCells) -> None:
        """The cells another object read, added in (`epik_amd_taxonomy_add_cells`): several devices summed into one."""
        shape = (self.num_samples, self.num_taxa)
        direct, assigned = (np.ascontiguousarray(a, dtype=U64) for a in (cells.direct, cells.assigned))
        totals = np.ascontiguousarray(cells.totals, dtype=capi.TAXA_TOTALS)
        if direct.shape != shape or assigned.shape != shape or totals.shape != (self.num_samples,):
            raise ValueError(f"cells must be {shape}")
        capi.check(self._lib.epik_amd_taxonomy_add_cells(self._handle, direct.ctypes.data, assigned.ctypes.data, totals.ctypes.data))


# -- the three files (epik_amd/host/taxonomy.cpp formats the same bytes) ---------------------------------------------
TAXA_COLUMNS = "assigned\tclade_assigned\tmass_q\tclade_mass_q\tmass\tclade_mass\ttaxopath"
COHORT_TAXA_COLUMNS = "name\tassigned\tclade_assigned\tmass_q\tclade_mass_q\ttaxopath"
READS_COLUMNS = "name\tshare\ttaxopath\tfirst_taxopath"


def _records_of(totals) -> int:
    return sum(int(totals[k]) for k in ("placed", "no_hit", "too_short", "too_narrow", "no_mass")) & 0xFFFFFFFFFFFFFFFF


def format_taxa_tsv(direct, assigned, totals, taxa: Taxonomy, tau_q: int) -> str:
    """taxa_<input>.tsv of one sample: direct[T], assigned[T] and its totals record.  A line for every taxon whose clade
    has a non-zero cell, in id order; the root's taxopath is `-`."""
    T = taxa.num_taxa
    clade_a, clade_m = clade_sums(assigned, taxa.first), clade_sums(direct, taxa.first)
    scale = float(1 << LWR_BITS)
    lines = [f"# epik_amd taxa v1\ttau_q={int(tau_q)}\ttaxa={T}",
             f"# records={_records_of(totals)}\tplaced={int(totals['placed'])}\tno_hit={int(totals['no_hit'])}"
             f"\ttoo_short={int(totals['too_short'])}\ttoo_narrow={int(totals['too_narrow'])}\tno_mass={int(totals['no_mass'])}",
             TAXA_COLUMNS]
    for t in range(T):
        if int(clade_a[t]) == 0 and int(clade_m[t]) == 0:
            continue
        m, cm = int(direct[t]), int(clade_m[t])
        lines.append(f"{int(assigned[t])}\t{int(clade_a[t])}\t{m}\t{cm}\t{float(m) / scale:.9f}\t{float(cm) / scale:.9f}\t{taxa.path[t] or '-'}")
    return "\n".join(lines) + "\n"


def format_cohort_taxa_tsv(names, cells: TaxaCells, taxa: Taxonomy, tau_q: int) -> str:
    """cohort_taxa_<list>.tsv: long format, list order, then taxon id, one line for every non-zero clade cell."""
    lines = [f"# epik_amd cohort taxa v1\ttau_q={int(tau_q)}\ttaxa={taxa.num_taxa}\tsamples={len(names)}", COHORT_TAXA_COLUMNS]
    clade_a, clade_m = clade_sums(cells.assigned, taxa.first), clade_sums(cells.direct, taxa.first)
    for s, name in enumerate(names):
        for t in range(taxa.num_taxa):
            if int(clade_a[s, t]) == 0 and int(clade_m[s, t]) == 0:
                continue
            lines.append(f"{name}\t{int(cells.assigned[s, t])}\t{int(clade_a[s, t])}\t{int(cells.direct[s, t])}\t{int(clade_m[s, t])}"
                         f"\t{taxa.path[t] or '-'}")
    return "\n".join(lines) + "\n"


def format_taxa_reads_tsv(names, records, taxa: Taxonomy, tau_q: int) -> str:
    """taxa_reads_<input>.tsv: per input record `name share taxopath first_taxopath`; share = taxon_mass_q / total_q as
    doubles, written %.17g; the class word stands in the taxopath column where there is no taxon."""
    lines = [f"# epik_amd taxa reads v1\ttau_q={int(tau_q)}\trecords={len(names)}", READS_COLUMNS]
    for name, rec in zip(names, records):
        taxon = int(rec["taxon"])
        if taxon in capi.TAXON_CLASSES:
            lines.append(f"{name}\t0\t{capi.TAXON_CLASSES[taxon]}\t-")
            continue
        share = float(int(rec["taxon_mass_q"])) / float(int(rec["total_q"]))
        lines.append(f"{name}\t{share:.17g}\t{taxa.path[taxon] or '-'}\t{taxa.path[int(rec['first_taxon'])] or '-'}")
    return "\n".join(lines) + "\n"
