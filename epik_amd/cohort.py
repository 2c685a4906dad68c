"""A cohort of samples placed on one tree (`epik_amd_cohort`, include/epik_amd.h): per sample the cells of a profile
(`mass`, `best`, totals), summed on the device from the rows a placement left there with a sample per read, and the
phylogenetic Kantorovich-Rubinstein distance between every two samples, computed there from those cells.  Integers
and a strictly sequential sum per pair: the same bits whatever the order, the grid, the stream or the devices.

`Cohort` is the ctypes side of the device object; `kr_host` the rule on the host (no device); `first_of` gives the
first[] of a tree from its parents; `format_*` / `read_*` are the files the drivers write with --cohort
(epik_amd/host/cohort.cpp and main.cpp write the same bytes).

Squash clustering of the samples (the header's second rule): `Cohort.squash` / `squash_device` on the device,
`squash_host` on the host, each giving the merge records (`capi.SQUASH_MERGE`); `format_squash_tsv`,
`format_squash_newick` and `read_squash_tsv` are the two files of --cohort-squash.

Edge principal components of the samples (the header's third rule): `Cohort.epca` / `epca_device` on the device,
`epca_host` on the host, each giving an `Epca`; `format_epca_tsv`, `format_epca_edges_tsv` and their readers are the two
files of --cohort-epca.

Phylogenetic k-means of the samples (the header's fourth rule): `Cohort.kmeans` / `kmeans_device` on the device,
`kmeans_host` on the host, each giving a `Kmeans`; `format_kmeans_tsv`, `format_kmeans_centroids_tsv` and their readers are
the two files of --cohort-kmeans.

Alpha diversity and rarefaction curves of the samples (the header's fifth rule): `Cohort.alpha` / `alpha_device` and
`Cohort.rarefy` / `rarefy_device` on the device, `alpha_host` and `rarefy_host` on the host; `format_alpha_tsv`,
`format_rarefy_tsv` and their readers are the files of --cohort-alpha and --cohort-rarefy.

Edge correlation with per-sample metadata and edge dispersion (the header's sixth rule): `Cohort.correlation` /
`correlation_device` and `Cohort.dispersion` / `dispersion_device` on the device, `correlation_host` and `dispersion_host`
on the host; `read_metadata` reads the file of --cohort-correlation; `format_correlation_tsv`, `format_dispersion_tsv` and
their readers are the files of --cohort-correlation and --cohort-dispersion.

PERMANOVA of the samples' groups over the KR distances (the header's seventh rule): `Cohort.permanova` /
`permanova_device` on the device, `permanova_host` and `permanova_kr_host` on the host; `read_factors` reads the file of
--cohort-permanova; `format_permanova_tsv` and `read_permanova_tsv` are its output file.
PERMDISP, the test of the groups' dispersions that goes with it (the header's PERMDISP rule): `Cohort.permdisp` /
`permdisp_device` on the device, `permdisp_host` and `permdisp_kr_host` on the host; `format_permdisp_tsv` is its output file.

The Mantel and partial Mantel tests and ANOSIM (the header's Mantel rule): `Cohort.mantel` / `mantel_device` and `Cohort.anosim` /
`anosim_device` on the device, `mantel_host`, `mantel_kr_host`, `anosim_host` and `anosim_kr_host` on the host, giving a `Mantel`
or an `Anosim`; the sides are columns of per-sample numbers and square matrices, `strata=` an argument of every form.

The edge test (the header's eighth rule): which branches differ between the groups of a factor column, by permutation with
the max-statistic adjustment: `Cohort.edgetest` / `edgetest_device` on the device, `edgetest_host` on the host;
`read_factors(..., most=32)` reads the file of --cohort-edge-test; `format_edgetest_tsv` and `read_edgetest_tsv` are its
output file.

Principal coordinates of the samples over the KR distances (the header's ninth rule): `Cohort.pcoa` / `pcoa_device` on the
device, `pcoa_host` and `pcoa_kr_host` on the host, each giving a `Pcoa` with all eigenvalues, the negative ones included;
`format_pcoa_tsv` and `read_pcoa_tsv` are the file of --cohort-pcoa.

The UniFrac distances between every two samples (the header's UniFrac rule; `DISTANCES` names them): `Cohort.unifrac` /
`unifrac_device` on the device, `unifrac_host` on the host; `format_unifrac_tsv` and `read_unifrac_tsv` are the files of
--cohort-unifrac.  PERMANOVA, PERMDISP and the principal coordinates take `metric=` (a name of `DISTANCES` or its number,
KR by default): the distance they run over, which --cohort-distance chooses and their files' first line then names.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import capi
from .profile import TOTALS

import re

SQUASH_HEADER = "step\tnode\ta\tb\tsize\tdist\tlen_a\tlen_b"
SAMPLES_HEADER = "name\trecords\tplaced\tno_hit\ttoo_short\ttoo_narrow\ttotal_mass_q"
PROFILE_HEADER = "name\tedge_num\tbest\tmass_q"
_TOTALS_DTYPE = np.dtype([(k, "<u8") for k in TOTALS])


def first_of(parent) -> np.ndarray:
    """first[b] = b - size[b] + 1 of every post-order id, from parent[] (the root's: -1 or capi.TREE_NO_PARENT)."""
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    first = np.arange(n, dtype=np.int64)
    for b in range(n - 1):
        p = int(parent[b])
        if not b < p < n:
            raise ValueError(f"branch {b}: the parent {p} is not above its child")
        first[p] = min(first[p], first[b])
    return first.astype(np.uint32)


def kr_host(mass, first, branch_length) -> np.ndarray:
    """KR(s, t) of the rule for mass[S][N] on the host (`epik_amd_cohort_kr_host`): float64 [S][S]."""
    lib = capi.load()
    mass = np.ascontiguousarray(mass, dtype=np.uint64)
    if mass.ndim != 2:
        raise ValueError("mass must be [num_samples][num_branches]")
    first = np.ascontiguousarray(first, dtype=np.uint32)
    length = np.ascontiguousarray(branch_length, dtype=np.float64)
    s, n = mass.shape
    if first.shape != (n,) or length.shape != (n,):
        raise ValueError(f"first and branch_length must hold one value per branch ({n})")
    out = np.full((s, s), np.nan, dtype=np.float64)
    capi.check(lib.epik_amd_cohort_kr_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, out.ctypes.data))
    return out


#: the distances by their number (EPIK_AMD_DISTANCE_*): KR and the three UniFrac distances
DISTANCES = ("kr", "unweighted", "weighted", "generalized")


def metric_id(metric) -> int:
    """EPIK_AMD_DISTANCE_* of a name of `DISTANCES`; a number is passed on as it is (the library refuses a bad one)."""
    if isinstance(metric, str):
        if metric not in DISTANCES:
            raise ValueError(f"unknown distance {metric!r} (one of {', '.join(DISTANCES)})")
        return DISTANCES.index(metric)
    metric = int(metric)
    if not 0 <= metric <= 0xffffffff:
        raise ValueError(f"metric = {metric} is no uint32")
    return metric


def unifrac_host(mass, first, branch_length, metric) -> np.ndarray:
    """The UniFrac distance `metric` of the rule for mass[S][N] on the host (`epik_amd_cohort_unifrac_host`): float64
    [S][S]."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    out = np.full((s, s), np.nan, dtype=np.float64)
    capi.check(lib.epik_amd_cohort_unifrac_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, metric_id(metric),
                                                out.ctypes.data))
    return out


def _cells_and_tree(mass, first, branch_length):
    mass = np.ascontiguousarray(mass, dtype=np.uint64)
    if mass.ndim != 2:
        raise ValueError("mass must be [num_samples][num_branches]")
    first = np.ascontiguousarray(first, dtype=np.uint32)
    length = np.ascontiguousarray(branch_length, dtype=np.float64)
    if first.shape != (mass.shape[1],) or length.shape != (mass.shape[1],):
        raise ValueError(f"first and branch_length must hold one value per branch ({mass.shape[1]})")
    return mass, first, length


def squash_host(mass, first, branch_length) -> np.ndarray:
    """The squash clustering of the rule for mass[S][N] on the host (`epik_amd_cohort_squash_host`): the records of the
    merges made, `capi.SQUASH_MERGE` [num_merges]."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    merges = np.zeros(max(s - 1, 0), dtype=capi.SQUASH_MERGE)
    count = ctypes.c_uint32(0xFFFFFFFF)
    capi.check(lib.epik_amd_cohort_squash_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data,
                                               merges.ctypes.data if s > 1 else None, ctypes.byref(count)))
    return _merges_made(merges, count.value)


def _merges_made(merges, count):
    """The first `count` records; the rest must be as the rule leaves them."""
    rest = merges[count:]
    if count > len(merges) or not ((rest["a"] == capi.SQUASH_NONE) & (rest["b"] == capi.SQUASH_NONE)).all() or \
            rest["dist"].view(np.uint64).any() or rest["len_a"].view(np.uint64).any() or rest["len_b"].view(np.uint64).any():
        raise RuntimeError("squash: the records past num_merges are not the unused record")
    return merges[:count].copy()


@dataclass
class Epca:
    """Edge principal components as the rule leaves them: `mu` float64 [K], `proj` float64 [S][K], `edge` float64 [K][N]
    and `info`, one `capi.EPCA_INFO` record (used, components, sweeps, converged, trace, scale)."""

    mu: np.ndarray
    proj: np.ndarray
    edge: np.ndarray
    info: np.ndarray

    @property
    def components(self) -> int:
        return int(self.info["components"])

    def null(self) -> np.ndarray:
        """Per component k < components whether it is null: !(mu_k > 2^-40 * scale)."""
        return ~(self.mu[:self.components] > np.ldexp(1.0, -40) * float(self.info["scale"]))


def _components(num_components) -> int:
    k = int(num_components)
    if not 0 <= k <= 0xFFFFFFFF:
        raise ValueError("num_components must fit 32 bits")
    return k


def _epca_buffers(s, n, k):
    k = max(k, 1)            # (a refused K still needs somewhere to point)
    return Epca(np.full(k, np.nan), np.full((s, k), np.nan), np.full((k, n), np.nan), np.zeros(1, dtype=capi.EPCA_INFO))


def epca_host(mass, first, num_components: int = 5) -> Epca:
    """The edge principal components of the rule for mass[S][N] on the host (`epik_amd_cohort_epca_host`)."""
    lib = capi.load()
    mass = np.ascontiguousarray(mass, dtype=np.uint64)
    if mass.ndim != 2:
        raise ValueError("mass must be [num_samples][num_branches]")
    first = np.ascontiguousarray(first, dtype=np.uint32)
    if first.shape != (mass.shape[1],):
        raise ValueError(f"first must hold one value per branch ({mass.shape[1]})")
    s, n = mass.shape
    k = _components(num_components)
    out = _epca_buffers(s, n, k)
    capi.check(lib.epik_amd_cohort_epca_host(mass.ctypes.data, s, n, first.ctypes.data, k, out.mu.ctypes.data,
                                             out.proj.ctypes.data, out.edge.ctypes.data, out.info.ctypes.data))
    out.info = out.info[0]
    return out


@dataclass
class Pcoa:
    """Principal coordinates as the rule leaves them: `mu` float64 [S] (all L eigenvalues by (mu descending, j ascending),
    the negative ones included, +0.0 beyond), `coord` float64 [S][K] and `info`, one `capi.PCOA_INFO` record (used,
    components, sweeps, converged, trace, scale, pos, neg)."""

    mu: np.ndarray
    coord: np.ndarray
    info: np.ndarray

    @property
    def components(self) -> int:
        return int(self.info["components"])

    def kinds(self) -> list:
        """Per eigenvalue k < used its class: "real" (mu_k > 2^-40 * scale), "negative" (mu_k < -2^-40 * scale) or "null"."""
        floor = np.ldexp(1.0, -40) * float(self.info["scale"])
        return ["real" if m > floor else "negative" if m < -floor else "null" for m in self.mu[:int(self.info["used"])]]

    @property
    def negative(self) -> float:
        """-neg / pos, 0 when pos is 0: how far the distances are from Euclidean."""
        pos, neg = float(self.info["pos"]), float(self.info["neg"])
        return (0.0 - neg) / pos if pos != 0 else 0.0


def _pcoa_buffers(s, k):
    k = max(k, 1)            # (a refused K still needs somewhere to point)
    return Pcoa(np.full(s, np.nan), np.full((s, k), np.nan), np.zeros(1, dtype=capi.PCOA_INFO))


def pcoa_kr_host(kr, totals, num_components: int = 5) -> Pcoa:
    """The principal coordinates of the rule from a KR matrix kr[S][S] and totals[S] (T_s) on the host
    (`epik_amd_cohort_pcoa_kr_host`)."""
    lib = capi.load()
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    if kr.ndim != 2 or kr.shape[0] != kr.shape[1]:
        raise ValueError("kr must be [num_samples][num_samples]")
    s = kr.shape[0]
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    if totals.shape != (s,):
        raise ValueError("one total mass per sample")
    k = _components(num_components)
    out = _pcoa_buffers(s, k)
    capi.check(lib.epik_amd_cohort_pcoa_kr_host(kr.ctypes.data, totals.ctypes.data, s, k, out.mu.ctypes.data, out.coord.ctypes.data,
                                                out.info.ctypes.data))
    out.info = out.info[0]
    return out


def pcoa_host(mass, first, branch_length, num_components: int = 5, metric="kr") -> Pcoa:
    """The principal coordinates of the rule for mass[S][N] over the distance `metric` on the host
    (`epik_amd_cohort_pcoa_metric_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    k = _components(num_components)
    out = _pcoa_buffers(s, k)
    capi.check(lib.epik_amd_cohort_pcoa_metric_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, metric_id(metric), k,
                                                    out.mu.ctypes.data, out.coord.ctypes.data, out.info.ctypes.data))
    out.info = out.info[0]
    return out


@dataclass
class Kmeans:
    """Phylogenetic k-means as the rule leaves it: `samples` `capi.KMEANS_SAMPLE` [S], `clusters` `capi.KMEANS_CLUSTER`
    [K], `centroids` float64 [K][N] and `info`, one `capi.KMEANS_INFO` record (used, clusters, iterations, converged)."""

    samples: np.ndarray
    clusters: np.ndarray
    centroids: np.ndarray
    info: np.ndarray

    @property
    def num_clusters(self) -> int:
        return int(self.info["clusters"])


def _count32(value, what) -> int:
    v = int(value)
    if not 0 <= v <= 0xFFFFFFFF:
        raise ValueError(f"{what} must fit 32 bits")
    return v


def _kmeans_buffers(s, n, k):
    k = min(max(k, 1), 0x10000)            # (a refused K still needs somewhere to point)
    return Kmeans(np.full(s, 0xAB, dtype=np.uint8).repeat(16).view(capi.KMEANS_SAMPLE),
                  np.full(k, 0xAB, dtype=np.uint8).repeat(24).view(capi.KMEANS_CLUSTER), np.full((k, n), np.nan),
                  np.zeros(1, dtype=capi.KMEANS_INFO))


def kmeans_host(mass, first, branch_length, num_clusters: int, max_iterations: int = 100) -> Kmeans:
    """The phylogenetic k-means of the rule for mass[S][N] on the host (`epik_amd_cohort_kmeans_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    k, m = _count32(num_clusters, "num_clusters"), _count32(max_iterations, "max_iterations")
    out = _kmeans_buffers(s, n, k)
    capi.check(lib.epik_amd_cohort_kmeans_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, k, m,
                                               out.samples.ctypes.data, out.clusters.ctypes.data, out.centroids.ctypes.data,
                                               out.info.ctypes.data))
    out.info = out.info[0]
    return out


def alpha_host(mass, first, branch_length) -> np.ndarray:
    """The alpha diversity indices of the rule for mass[S][N] on the host (`epik_amd_cohort_alpha_host`): `capi.ALPHA` [S]."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    out = np.full(s * 5, np.nan).view(capi.ALPHA)
    capi.check(lib.epik_amd_cohort_alpha_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, out.ctypes.data))
    return out


def _curve_buffer(s, num_depths) -> np.ndarray:
    return np.full((s, min(max(num_depths, 1), 0x10000), 2), np.nan)   # (refused depths still need somewhere to point)


def rarefy_host(best, first, branch_length, depth_step: int, num_depths: int) -> np.ndarray:
    """The rarefaction curves of the rule for best[S][N] on the host (`epik_amd_cohort_rarefy_host`): float64 [S][J][2],
    the expected unrooted and rooted PD of k_j = j * depth_step reads, {-1, -1} beyond a sample's reads."""
    lib = capi.load()
    best, first, length = _cells_and_tree(best, first, branch_length)
    s, n = best.shape
    step, depths = _count32(depth_step, "depth_step"), _count32(num_depths, "num_depths")
    out = _curve_buffer(s, depths)
    capi.check(lib.epik_amd_cohort_rarefy_host(best.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, step, depths,
                                               out.ctypes.data))
    return out


def _mass_and_first(mass, first):
    mass = np.ascontiguousarray(mass, dtype=np.uint64)
    if mass.ndim != 2:
        raise ValueError("mass must be [num_samples][num_branches]")
    first = np.ascontiguousarray(first, dtype=np.uint32)
    if first.shape != (mass.shape[1],):
        raise ValueError(f"first must hold one value per branch ({mass.shape[1]})")
    return mass, first


def _metadata(meta, num_samples: int) -> np.ndarray:
    meta = np.ascontiguousarray(meta, dtype=np.float64)
    if meta.ndim != 2 or meta.shape[0] != num_samples:
        raise ValueError(f"meta must be [num_samples = {num_samples}][num_columns]")
    return meta


def _na(count: int, dtype) -> np.ndarray:
    return np.full(count * len(dtype.names), np.nan).view(dtype)


def correlation_host(mass, first, meta):
    """The edge correlation of the rule for mass[S][N] and meta[S][M] (NaN: missing) on the host
    (`epik_amd_cohort_correlation_host`): (`capi.CORRELATION` [M][N], used uint32 [M])."""
    lib = capi.load()
    mass, first = _mass_and_first(mass, first)
    s, n = mass.shape
    meta = _metadata(meta, s)
    m = meta.shape[1]
    out, used = _na(max(m, 1) * n, capi.CORRELATION), np.zeros(max(m, 1), dtype=np.uint32)
    capi.check(lib.epik_amd_cohort_correlation_host(mass.ctypes.data, s, n, first.ctypes.data, meta.ctypes.data, m,
                                                    out.ctypes.data, used.ctypes.data))
    return out.reshape(max(m, 1), n), used


def dispersion_host(mass, first) -> np.ndarray:
    """The edge dispersion of the rule for mass[S][N] on the host (`epik_amd_cohort_dispersion_host`): `capi.DISPERSION` [N]."""
    lib = capi.load()
    mass, first = _mass_and_first(mass, first)
    s, n = mass.shape
    out = _na(n, capi.DISPERSION)
    capi.check(lib.epik_amd_cohort_dispersion_host(mass.ctypes.data, s, n, first.ctypes.data, out.ctypes.data))
    return out


@dataclass
class Permanova:
    """What PERMANOVA gives: `records` `capi.PERMANOVA` [M][1 + Q] (slot 0 the whole column, the pair (g, h) at
    `pair_slot(g, h)`; Q = 496 with pairwise, else 0), `ssw` float64 [M][1 + Q][P + 1] (SSW of permutation 0 .. P; None
    where not asked for) and `group_ss` float64 [M][256] (W_g / n_g of the observed labelling)."""
    records: np.ndarray
    ssw: np.ndarray | None
    group_ss: np.ndarray


def pair_slot(g: int, h: int) -> int:
    """The slot of the pair of groups g < h in a column's row of tests."""
    if not 0 <= g < h < capi.PERMANOVA_MAX_PAIR_GROUPS:
        raise ValueError("a pair is g < h < 32")
    return 1 + h * (h - 1) // 2 + g


def _labels(labels, num_samples: int) -> np.ndarray:
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    if labels.ndim != 2 or labels.shape[0] != num_samples:
        raise ValueError(f"labels must be [num_samples = {num_samples}][num_columns]")
    return labels


#: the entry that takes strata, by the entry that a call without them goes through
_STRATA_ENTRY = {
    "permanova_device": "permanova_strata_device",
    "permanova_metric": "permanova_strata",
    "permanova_metric_host": "permanova_strata_host",
    "permanova_kr_host": "permanova_strata_kr_host",
    "permdisp_device": "permdisp_strata_device",
    "permdisp_metric": "permdisp_strata",
    "permdisp_metric_host": "permdisp_strata_host",
    "permdisp_kr_host": "permdisp_strata_kr_host",
    "model_device": "model_strata_device",
    "model_metric": "model_strata",
    "model_metric_host": "model_strata_host",
    "model_kr_host": "model_strata_kr_host",
    "edgetest_device": "edgetest_strata_device",
    "edgetest": "edgetest_strata",
    "edgetest_host": "edgetest_strata_host",
    "edgemodel_device": "edgemodel_strata_device",
    "edgemodel": "edgemodel_strata",
    "edgemodel_host": "edgemodel_strata_host",
}


def _call(lib, entry: str, strata, num_samples: int, *args) -> None:
    """`epik_amd_cohort_<entry>(*args)`, checked.  With `strata` (one id per sample, any uint32: the permutations stay
    within them, the strata rule of include/epik_amd.h) its `_strata` sibling is called with them as the last argument;
    without, the entry itself, as before."""
    if strata is None:
        capi.check(getattr(lib, "epik_amd_cohort_" + entry)(*args))
        return
    strata = np.ascontiguousarray(strata, dtype=np.uint32)
    if strata.shape != (num_samples,):
        raise ValueError(f"strata must be [num_samples = {num_samples}]")
    capi.check(getattr(lib, "epik_amd_cohort_" + _STRATA_ENTRY[entry])(*args, strata.ctypes.data))


def _permanova_buffers(m: int, permutations: int, pairwise: bool, with_ssw: bool):
    slots = 1 + (capi.PERMANOVA_PAIR_SLOTS if pairwise else 0)
    records = np.zeros((max(m, 1), slots), dtype=capi.PERMANOVA)
    ssw = np.full((max(m, 1), slots, min(max(int(permutations), 0), capi.PERMANOVA_MAX_PERMUTATIONS) + 1), np.nan) if with_ssw else None
    return records, ssw, np.full((max(m, 1), capi.PERMANOVA_MAX_GROUPS), np.nan)


def permanova_kr_host(kr, totals, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                      with_ssw: bool = True, strata=None) -> Permanova:
    """PERMANOVA of the rule from a KR matrix kr[S][S] and totals[S] (T_s) on the host
    (`epik_amd_cohort_permanova_kr_host`)."""
    lib = capi.load()
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    if kr.ndim != 2 or kr.shape[0] != kr.shape[1]:
        raise ValueError("kr must be [num_samples][num_samples]")
    s = kr.shape[0]
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    if totals.shape != (s,):
        raise ValueError("one total mass per sample")
    labels = _labels(labels, s)
    records, ssw, group_ss = _permanova_buffers(labels.shape[1], permutations, pairwise, with_ssw)
    _call(lib, "permanova_kr_host", strata, s, kr.ctypes.data, totals.ctypes.data, s, labels.ctypes.data, labels.shape[1],
          int(permutations), int(seed), int(bool(pairwise)), records.ctypes.data,
          ssw.ctypes.data if with_ssw else None, group_ss.ctypes.data)
    return Permanova(records, ssw, group_ss)


def permanova_host(mass, first, branch_length, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                   with_ssw: bool = True, metric="kr", strata=None) -> Permanova:
    """PERMANOVA of the rule for mass[S][N] and labels[S][M] (0xffffffff: missing) over the distance `metric` on the host
    (`epik_amd_cohort_permanova_metric_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    labels = _labels(labels, s)
    records, ssw, group_ss = _permanova_buffers(labels.shape[1], permutations, pairwise, with_ssw)
    _call(lib, "permanova_metric_host", strata, s, mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data,
          metric_id(metric), labels.ctypes.data, labels.shape[1], int(permutations),
          int(seed), int(bool(pairwise)), records.ctypes.data,
          ssw.ctypes.data if with_ssw else None, group_ss.ctypes.data)
    return Permanova(records, ssw, group_ss)


@dataclass
class Permdisp:
    """What PERMDISP gives: `records` `capi.PERMDISP` [M][1 + Q] (the slots of `Permanova`), `stat` float64 [M][1 + Q][P + 1]
    (eta2 in slot 0, eta_r of the permutations 1 .. P; None where not asked for), `group_mean` float64 [M][32] (the mean
    distance to centroid of every group) and `z` float64 [M][S] (the distances by sample, NA outside U_c)."""
    records: np.ndarray
    stat: np.ndarray | None
    group_mean: np.ndarray
    z: np.ndarray


def _permdisp_buffers(m: int, s: int, permutations: int, pairwise: bool, with_stat: bool) -> Permdisp:
    slots = 1 + (capi.PERMDISP_PAIR_SLOTS if pairwise else 0)
    records = np.zeros((max(m, 1), slots), dtype=capi.PERMDISP)
    stat = np.full((max(m, 1), slots, min(max(int(permutations), 0), capi.PERMDISP_MAX_PERMUTATIONS) + 1), np.nan) if with_stat else None
    return Permdisp(records, stat, np.full((max(m, 1), capi.PERMDISP_MAX_GROUPS), np.nan), np.full((max(m, 1), s), np.nan))


def permdisp_kr_host(kr, totals, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                     with_stat: bool = True, strata=None) -> Permdisp:
    """PERMDISP of the rule from a KR matrix kr[S][S] and totals[S] (T_s) on the host (`epik_amd_cohort_permdisp_kr_host`)."""
    lib = capi.load()
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    if kr.ndim != 2 or kr.shape[0] != kr.shape[1]:
        raise ValueError("kr must be [num_samples][num_samples]")
    s = kr.shape[0]
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    if totals.shape != (s,):
        raise ValueError("one total mass per sample")
    labels = _labels(labels, s)
    out = _permdisp_buffers(labels.shape[1], s, permutations, pairwise, with_stat)
    _call(lib, "permdisp_kr_host", strata, s, kr.ctypes.data, totals.ctypes.data, s, labels.ctypes.data, labels.shape[1],
          int(permutations), int(seed), int(bool(pairwise)), out.records.ctypes.data,
          out.stat.ctypes.data if with_stat else None, out.group_mean.ctypes.data,
          out.z.ctypes.data)
    return out


def permdisp_host(mass, first, branch_length, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                  with_stat: bool = True, metric="kr", strata=None) -> Permdisp:
    """PERMDISP of the rule for mass[S][N] and labels[S][M] (0xffffffff: missing) over the distance `metric` on the host
    (`epik_amd_cohort_permdisp_metric_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    labels = _labels(labels, s)
    out = _permdisp_buffers(labels.shape[1], s, permutations, pairwise, with_stat)
    _call(lib, "permdisp_metric_host", strata, s, mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data,
          metric_id(metric), labels.ctypes.data, labels.shape[1], int(permutations),
          int(seed), int(bool(pairwise)), out.records.ctypes.data,
          out.stat.ctypes.data if with_stat else None, out.group_mean.ctypes.data,
          out.z.ctypes.data)
    return out


@dataclass
class Mantel:
    """What the Mantel tests give: `records` `capi.MANTEL` [tests], the tests in side-major order, pearson before spearman
    (`side`, `method` and `partial` name each), and `stat` float64 [tests][P + 1] (the statistic of permutation 0 .. P; None
    where not asked for)."""
    records: np.ndarray
    stat: np.ndarray | None


@dataclass
class Anosim:
    """What ANOSIM gives: `records` `capi.ANOSIM` [M] and `stat` float64 [M][P + 1] (R of permutation 0 .. P; None where not
    asked for)."""
    records: np.ndarray
    stat: np.ndarray | None


def _strata(strata, num_samples: int):
    if strata is None:
        return None
    strata = np.ascontiguousarray(strata, dtype=np.uint32)
    if strata.shape != (num_samples,):
        raise ValueError(f"strata must be [num_samples = {num_samples}]")
    return strata


def _pointer(array):
    return array.ctypes.data if array is not None and array.size else None


def _sides(values, matrices, matrix_present, methods, control, permutations, num_samples: int, with_stat: bool):
    """The sides of a Mantel call as the C ABI takes them: (the arrays, which must outlive the call; the arguments from `values`
    to `num_permutations`; an empty `Mantel`).  values [Mv][S] (NaN: missing), matrices [Mm][S][S], matrix_present [Mm][S]
    (all present if None); `methods` names of `capi.MANTEL_METHODS` (or their bits), `control` a side index or None."""
    s = num_samples
    values = np.zeros((0, s)) if values is None else np.ascontiguousarray(values, dtype=np.float64)
    matrices = np.zeros((0, s, s)) if matrices is None else np.ascontiguousarray(matrices, dtype=np.float64)
    if values.ndim != 2 or values.shape[1] != s:
        raise ValueError(f"values must be [num_columns][num_samples = {s}]")
    if matrices.ndim != 3 or matrices.shape[1:] != (s, s):
        raise ValueError(f"matrices must be [num_matrices][{s}][{s}]")
    present = np.ones(matrices.shape[:2], np.uint8) if matrix_present is None else np.ascontiguousarray(matrix_present, dtype=np.uint8)
    if present.shape != matrices.shape[:2]:
        raise ValueError("matrix_present must be [num_matrices][num_samples]")
    bits = int(methods) if isinstance(methods, (int, np.integer)) else 0
    if not isinstance(methods, (int, np.integer)):
        for name in ((methods,) if isinstance(methods, str) else methods):
            if name not in capi.MANTEL_METHODS:
                raise ValueError(f"unknown method {name!r} (pearson or spearman)")
            bits |= capi.MANTEL_METHODS[name]
    control = capi.MANTEL_NO_CONTROL if control is None else int(control)
    if not 0 <= control <= 0xFFFFFFFF or not 0 <= bits <= 0xFFFFFFFF:
        raise ValueError("control and methods are uint32")
    tests = max((len(values) + len(matrices)) * bin(bits & 3).count("1"), 1)
    rows = min(max(int(permutations), 0), capi.PERMANOVA_MAX_PERMUTATIONS) + 1
    out = Mantel(np.zeros(tests, dtype=capi.MANTEL), np.full((tests, rows), np.nan) if with_stat else None)
    args = (_pointer(values), len(values), _pointer(matrices), _pointer(present), len(matrices), bits, control, int(permutations))
    return (values, matrices, present), args, out


def _kr_and_totals(kr, totals):
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    if kr.ndim != 2 or kr.shape[0] != kr.shape[1]:
        raise ValueError("kr must be [num_samples][num_samples]")
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    if totals.shape != (kr.shape[0],):
        raise ValueError("one total mass per sample")
    return kr, totals


def mantel_kr_host(kr, totals, values=None, matrices=None, matrix_present=None, methods=("pearson",), control=None,
                   permutations: int = 999, seed: int = 1, strata=None, with_stat: bool = True) -> Mantel:
    """The Mantel and partial Mantel tests of the rule from a matrix kr[S][S] and totals[S] (T_s) on the host
    (`epik_amd_cohort_mantel_kr_host`): every side against the matrix, with `control` (a side) held fixed."""
    lib = capi.load()
    kr, totals = _kr_and_totals(kr, totals)
    s = kr.shape[0]
    keep, args, out = _sides(values, matrices, matrix_present, methods, control, permutations, s, with_stat)
    strata = _strata(strata, s)
    capi.check(lib.epik_amd_cohort_mantel_kr_host(kr.ctypes.data, totals.ctypes.data, s, *args, int(seed), _pointer(strata),
                                                  out.records.ctypes.data, _pointer(out.stat)))
    return out


def mantel_host(mass, first, branch_length, values=None, matrices=None, matrix_present=None, methods=("pearson",), control=None,
                permutations: int = 999, seed: int = 1, metric="kr", strata=None, with_stat: bool = True) -> Mantel:
    """The same for mass[S][N] over the distance `metric` on the host (`epik_amd_cohort_mantel_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    keep, args, out = _sides(values, matrices, matrix_present, methods, control, permutations, s, with_stat)
    strata = _strata(strata, s)
    capi.check(lib.epik_amd_cohort_mantel_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, metric_id(metric), *args,
                                               int(seed), _pointer(strata), out.records.ctypes.data, _pointer(out.stat)))
    return out


def _anosim_buffers(m: int, permutations: int, with_stat: bool) -> Anosim:
    rows = min(max(int(permutations), 0), capi.PERMANOVA_MAX_PERMUTATIONS) + 1
    return Anosim(np.zeros(max(m, 1), dtype=capi.ANOSIM), np.full((max(m, 1), rows), np.nan) if with_stat else None)


def anosim_kr_host(kr, totals, labels, permutations: int = 999, seed: int = 1, strata=None, with_stat: bool = True) -> Anosim:
    """ANOSIM of the rule from a matrix kr[S][S], totals[S] (T_s) and labels[S][M] (0xffffffff: missing) on the host
    (`epik_amd_cohort_anosim_kr_host`)."""
    lib = capi.load()
    kr, totals = _kr_and_totals(kr, totals)
    s = kr.shape[0]
    labels = _labels(labels, s)
    out = _anosim_buffers(labels.shape[1], permutations, with_stat)
    strata = _strata(strata, s)
    capi.check(lib.epik_amd_cohort_anosim_kr_host(kr.ctypes.data, totals.ctypes.data, s, labels.ctypes.data, labels.shape[1],
                                                  int(permutations), int(seed), _pointer(strata), out.records.ctypes.data,
                                                  _pointer(out.stat)))
    return out


def anosim_host(mass, first, branch_length, labels, permutations: int = 999, seed: int = 1, metric="kr", strata=None,
                with_stat: bool = True) -> Anosim:
    """The same for mass[S][N] over the distance `metric` on the host (`epik_amd_cohort_anosim_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    labels = _labels(labels, s)
    out = _anosim_buffers(labels.shape[1], permutations, with_stat)
    strata = _strata(strata, s)
    capi.check(lib.epik_amd_cohort_anosim_host(mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, metric_id(metric),
                                               labels.ctypes.data, labels.shape[1], int(permutations), int(seed), _pointer(strata),
                                               out.records.ctypes.data, _pointer(out.stat)))
    return out


@dataclass
class Model:
    """What the sequential model gives: `records` `capi.MODEL_TERM` [T + 1] (the terms in test order, then the whole model),
    `info` one `capi.MODEL_INFO`, `stat` float64 [T + 1][P + 1] (F of permutation 0 .. P; None where not asked for) and
    `aliased` uint8 [64] (1 for a column of the design that was dropped)."""
    records: np.ndarray
    info: np.void
    stat: np.ndarray | None
    aliased: np.ndarray


def _design(kind, labels, values, num_samples: int):
    """kind[T] (0 a factor, 1 numeric), labels[S][T] uint32 and values[S][T] float64 as the C ABI takes them."""
    kind = np.ascontiguousarray(kind, dtype=np.uint32)
    if kind.ndim != 1:
        raise ValueError("kind must be [num_terms]")
    shape = (num_samples, kind.shape[0])
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    values = np.ascontiguousarray(values, dtype=np.float64)
    if labels.shape != shape or values.shape != shape:
        raise ValueError(f"labels and values must be [num_samples = {num_samples}][num_terms = {kind.shape[0]}]")
    return kind, labels, values


def _model_buffers(t: int, permutations: int, with_stat: bool):
    records = np.zeros(max(t, 0) + 1, dtype=capi.MODEL_TERM)
    info = np.zeros(1, dtype=capi.MODEL_INFO)
    stat = np.full((max(t, 0) + 1, min(max(int(permutations), 0), capi.MODEL_MAX_PERMUTATIONS) + 1), np.nan) if with_stat else None
    return records, info, stat, np.zeros(capi.MODEL_MAX_COLUMNS, dtype=np.uint8)


def model_kr_host(kr, totals, kind, labels, values, permutations: int = 999, seed: int = 1, with_stat: bool = True,
                  strata=None) -> Model:
    """The sequential model of the rule from a distance matrix kr[S][S] and totals[S] (T_s) on the host
    (`epik_amd_cohort_model_kr_host`)."""
    lib = capi.load()
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    if kr.ndim != 2 or kr.shape[0] != kr.shape[1]:
        raise ValueError("kr must be [num_samples][num_samples]")
    s = kr.shape[0]
    totals = np.ascontiguousarray(totals, dtype=np.uint64)
    if totals.shape != (s,):
        raise ValueError("one total mass per sample")
    kind, labels, values = _design(kind, labels, values, s)
    records, info, stat, aliased = _model_buffers(kind.shape[0], permutations, with_stat)
    _call(lib, "model_kr_host", strata, s, kr.ctypes.data, totals.ctypes.data, s, kind.ctypes.data, labels.ctypes.data,
          values.ctypes.data, kind.shape[0], int(permutations), int(seed), records.ctypes.data,
          info.ctypes.data, stat.ctypes.data if with_stat else None, aliased.ctypes.data)
    return Model(records, info[0], stat, aliased)


def model_host(mass, first, branch_length, kind, labels, values, permutations: int = 999, seed: int = 1, with_stat: bool = True,
               metric="kr", strata=None) -> Model:
    """The sequential model of the rule for mass[S][N] and the design kind[T], labels[S][T] (0xffffffff: missing) and
    values[S][T] (NaN: missing) over the distance `metric` on the host (`epik_amd_cohort_model_metric_host`)."""
    lib = capi.load()
    mass, first, length = _cells_and_tree(mass, first, branch_length)
    s, n = mass.shape
    kind, labels, values = _design(kind, labels, values, s)
    records, info, stat, aliased = _model_buffers(kind.shape[0], permutations, with_stat)
    _call(lib, "model_metric_host", strata, s, mass.ctypes.data, s, n, first.ctypes.data, length.ctypes.data, metric_id(metric),
          kind.ctypes.data, labels.ctypes.data, values.ctypes.data, kind.shape[0],
          int(permutations), int(seed), records.ctypes.data, info.ctypes.data,
          stat.ctypes.data if with_stat else None, aliased.ctypes.data)
    return Model(records, info[0], stat, aliased)


@dataclass
class Edgetest:
    """What the edge test gives: `records` `capi.EDGETEST` [M][N], `stat` float64 [M][4][N][P + 1] (eta of the labellings
    0 .. P; None where not asked for) and `max` float64 [M][4][P + 1] (the maxima over a family's defined branches)."""
    records: np.ndarray
    stat: np.ndarray | None
    max: np.ndarray | None


def _edgetest_buffers(m: int, n: int, permutations: int, with_stat: bool, with_max: bool):
    row = min(max(int(permutations), 0), capi.EDGETEST_MAX_PERMUTATIONS) + 1
    records = np.zeros((max(m, 1), n), dtype=capi.EDGETEST)
    stat = np.full((max(m, 1), capi.EDGETEST_FAMILIES, n, row), np.nan) if with_stat else None
    return records, stat, np.full((max(m, 1), capi.EDGETEST_FAMILIES, row), np.nan) if with_max else None


def edgetest_host(mass, first, labels, permutations: int = 999, seed: int = 1, with_stat: bool = True,
                  with_max: bool = True, strata=None) -> Edgetest:
    """The edge test of the rule for mass[S][N] and labels[S][M] (0xffffffff: missing) on the host, one thread
    (`epik_amd_cohort_edgetest_host`)."""
    lib = capi.load()
    mass, first = _mass_and_first(mass, first)
    s, n = mass.shape
    labels = _labels(labels, s)
    records, stat, most = _edgetest_buffers(labels.shape[1], n, permutations, with_stat, with_max)
    _call(lib, "edgetest_host", strata, s, mass.ctypes.data, s, n, first.ctypes.data, labels.ctypes.data, labels.shape[1],
          int(permutations), int(seed), records.ctypes.data,
          stat.ctypes.data if with_stat else None, most.ctypes.data if with_max else None)
    return Edgetest(records, stat, most)


@dataclass
class Edgemodel:
    """What the edge model gives: `records` `capi.EDGEMODEL` [T][N] (a term a row, the families mass and imbalance), `info` one
    `capi.EDGEMODEL_INFO`, `stat` float64 [T][2][N][P + 1] (the partial R2 of the permutations 0 .. P; None where not asked
    for), `max` float64 [T][2][P + 1] (the maxima over the defined branches) and `aliased` uint8 [64] as the model's."""
    records: np.ndarray
    info: np.void
    stat: np.ndarray | None
    max: np.ndarray | None
    aliased: np.ndarray


def _edgemodel_buffers(t: int, n: int, permutations: int, with_stat: bool, with_max: bool):
    row = min(max(int(permutations), 0), capi.MODEL_MAX_PERMUTATIONS) + 1
    t = min(max(t, 1), capi.MODEL_MAX_TERMS)
    records = np.zeros((t, n), dtype=capi.EDGEMODEL)
    info = np.zeros(1, dtype=capi.EDGEMODEL_INFO)
    stat = np.full((t, capi.EDGEMODEL_FAMILIES, n, row), np.nan) if with_stat else None
    most = np.full((t, capi.EDGEMODEL_FAMILIES, row), np.nan) if with_max else None
    return records, info, stat, most, np.zeros(capi.MODEL_MAX_COLUMNS, dtype=np.uint8)


def edgemodel_host(mass, first, kind, labels, values, permutations: int = 999, seed: int = 1, with_stat: bool = True,
                   with_max: bool = True, strata=None) -> Edgemodel:
    """The edge model of the rule for mass[S][N] and the design kind[T], labels[S][T] (0xffffffff: missing) and values[S][T]
    (NaN: missing) on the host, one thread (`epik_amd_cohort_edgemodel_host`)."""
    lib = capi.load()
    mass, first = _mass_and_first(mass, first)
    s, n = mass.shape
    kind, labels, values = _design(kind, labels, values, s)
    records, info, stat, most, aliased = _edgemodel_buffers(kind.shape[0], n, permutations, with_stat, with_max)
    _call(lib, "edgemodel_host", strata, s, mass.ctypes.data, s, n, first.ctypes.data, kind.ctypes.data, labels.ctypes.data,
          values.ctypes.data, kind.shape[0], int(permutations), int(seed), records.ctypes.data, info.ctypes.data,
          stat.ctypes.data if with_stat else None, most.ctypes.data if with_max else None, aliased.ctypes.data)
    return Edgemodel(records, info[0], stat, most, aliased)


@dataclass
class CohortCells:
    """What a cohort holds on the host: `mass` and `best` uint64 [S][N], `totals` a record array [S] with the fields
    of `epik_amd_profile_totals`, and `bad_samples`."""

    mass: np.ndarray
    best: np.ndarray
    totals: np.ndarray
    bad_samples: int = 0

    def records(self) -> np.ndarray:
        t = self.totals
        return t["placed"] + t["no_hit"] + t["too_short"] + t["too_narrow"]


class Cohort:
    """A device cohort of `num_samples` samples for one placer (`epik_amd_cohort_create`): all zero at first.  A context
    manager; `close()` frees it."""

    def __init__(self, placer, num_samples: int):
        self._lib = capi.load()
        self._handle = ctypes.c_void_p()
        if not 0 <= int(num_samples) <= 0xFFFFFFFF:
            raise ValueError("num_samples must fit 32 bits")
        capi.check(self._lib.epik_amd_cohort_create(placer._handle, int(num_samples), ctypes.byref(self._handle)))
        self.device = placer.device
        self.num_samples = int(num_samples)
        self.num_branches = placer.num_branches
        self.keep_at_most = placer.keep_at_most

    def close(self) -> None:
        if getattr(self, "_handle", None):
            self._lib.epik_amd_cohort_destroy(self._handle)
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
        capi.check(self._lib.epik_amd_cohort_info(self._handle, None, None, ctypes.byref(lds)))
        return bool(lds.value)

    def add_device(self, d_rows: int, d_n_rows: int, d_kmer_counts: int, d_samples: int, n: int, d_weights: int = 0,
                   stream: int = 0) -> None:
        """Device pointers, asynchronous on `stream` (`epik_amd_cohort_add_device`): read i goes to row d_samples[i]
        (uint32); `d_weights` 0: every read once."""
        capi.check(self._lib.epik_amd_cohort_add_device(self._handle, d_rows or None, d_n_rows or None, d_kmer_counts or None,
                                                        d_weights or None, d_samples or None, int(n), stream or None))

    def read(self) -> CohortCells:
        """Synchronises the device and returns the cells (`epik_amd_cohort_read`)."""
        shape = (self.num_samples, self.num_branches)
        mass, best = np.zeros(shape, np.uint64), np.zeros(shape, np.uint64)
        totals = np.zeros(self.num_samples, dtype=_TOTALS_DTYPE)
        bad = ctypes.c_uint64(0)
        capi.check(self._lib.epik_amd_cohort_read(self._handle, mass.ctypes.data, best.ctypes.data, totals.ctypes.data,
                                                  ctypes.byref(bad)))
        return CohortCells(mass, best, totals, int(bad.value))

    def add_cells(self, mass=None, best=None, totals=None) -> None:
        """Host arrays of the shapes `read` gives (each may be None) added in: merging the cohorts of several devices."""
        shape = (self.num_samples, self.num_branches)
        ptrs = []
        keep = []
        for arr in (mass, best):
            if arr is None:
                ptrs.append(None)
                continue
            arr = np.ascontiguousarray(arr, dtype=np.uint64)
            if arr.shape != shape:
                raise ValueError(f"cells must be {shape}, not {arr.shape}")
            keep.append(arr)
            ptrs.append(arr.ctypes.data)
        if totals is None:
            ptrs.append(None)
        else:
            totals = np.ascontiguousarray(totals, dtype=_TOTALS_DTYPE)
            if totals.shape != (self.num_samples,):
                raise ValueError(f"totals must hold one record per sample ({self.num_samples})")
            keep.append(totals)
            ptrs.append(totals.ctypes.data)
        capi.check(self._lib.epik_amd_cohort_add_cells(self._handle, *ptrs))

    def _lengths(self, tree, branch_length) -> np.ndarray:
        length = np.ascontiguousarray(branch_length, dtype=np.float64)
        if length.shape != (self.num_branches,):
            raise ValueError(f"branch_length must hold one value per branch ({self.num_branches})")
        if tree is None or not getattr(tree, "_handle", None):
            raise ValueError("kr needs a device tree (Placer.tree)")
        return length

    def kr_device(self, tree, branch_length, d_out: int, stream: int = 0) -> None:
        """KR(s, t) into d_out, float64 [S][S] in device memory, every cell written; asynchronous on `stream` once the
        lengths (host) are copied (`epik_amd_cohort_kr_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_kr_device(self._handle, tree._handle, length.ctypes.data, d_out or None,
                                                       stream or None))

    def kr(self, tree, branch_length) -> np.ndarray:
        """KR(s, t) for all pairs, float64 [S][S] (`epik_amd_cohort_kr`)."""
        length = self._lengths(tree, branch_length)
        out = np.full((self.num_samples, self.num_samples), np.nan, dtype=np.float64)
        capi.check(self._lib.epik_amd_cohort_kr(self._handle, tree._handle, length.ctypes.data, out.ctypes.data))
        return out

    def unifrac_device(self, tree, branch_length, metric, d_out: int, stream: int = 0) -> None:
        """The UniFrac distance `metric` into d_out, float64 [S][S] in device memory, every cell written; asynchronous on
        `stream` once the lengths (host) are copied (`epik_amd_cohort_unifrac_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_unifrac_device(self._handle, tree._handle, length.ctypes.data, metric_id(metric),
                                                            d_out or None, stream or None))

    def unifrac(self, tree, branch_length, metric) -> np.ndarray:
        """The UniFrac distance `metric` for all pairs, float64 [S][S] (`epik_amd_cohort_unifrac`)."""
        length = self._lengths(tree, branch_length)
        out = np.full((self.num_samples, self.num_samples), np.nan, dtype=np.float64)
        capi.check(self._lib.epik_amd_cohort_unifrac(self._handle, tree._handle, length.ctypes.data, metric_id(metric),
                                                     out.ctypes.data))
        return out

    def squash_device(self, tree, branch_length, d_merges: int, d_num_merges: int, stream: int = 0) -> None:
        """The squash clustering into device memory: d_merges `capi.SQUASH_MERGE` [S - 1], every record written, and
        d_num_merges one uint32; asynchronous on `stream` once the lengths (host) are copied, all steps enqueued
        (`epik_amd_cohort_squash_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_squash_device(self._handle, tree._handle, length.ctypes.data, d_merges or None,
                                                           d_num_merges or None, stream or None))

    def squash(self, tree, branch_length) -> np.ndarray:
        """The records of the merges made, `capi.SQUASH_MERGE` [num_merges] (`epik_amd_cohort_squash`)."""
        length = self._lengths(tree, branch_length)
        merges = np.zeros(self.num_samples - 1, dtype=capi.SQUASH_MERGE)
        count = ctypes.c_uint32(0xFFFFFFFF)
        capi.check(self._lib.epik_amd_cohort_squash(self._handle, tree._handle, length.ctypes.data,
                                                    merges.ctypes.data if len(merges) else None, ctypes.byref(count)))
        return _merges_made(merges, count.value)

    def epca_device(self, tree, num_components: int, d_mu: int, d_proj: int, d_edge: int, d_info: int, stream: int = 0) -> None:
        """The edge principal components into device memory: d_mu float64 [K], d_proj float64 [S][K], d_edge float64
        [K][N], d_info one `capi.EPCA_INFO`, every cell written.  Synchronises `stream` once for the number of used
        samples and, on the eigensolver's global path, once per sweep (`epik_amd_cohort_epca_device`)."""
        if tree is None or not getattr(tree, "_handle", None):
            raise ValueError("epca needs a device tree (Placer.tree)")
        capi.check(self._lib.epik_amd_cohort_epca_device(self._handle, tree._handle, _components(num_components), d_mu or None,
                                                         d_proj or None, d_edge or None, d_info or None, stream or None))

    def epca(self, tree, num_components: int = 5) -> Epca:
        """The edge principal components of the samples, an `Epca` (`epik_amd_cohort_epca`)."""
        if tree is None or not getattr(tree, "_handle", None):
            raise ValueError("epca needs a device tree (Placer.tree)")
        k = _components(num_components)
        out = _epca_buffers(self.num_samples, self.num_branches, k)
        capi.check(self._lib.epik_amd_cohort_epca(self._handle, tree._handle, k, out.mu.ctypes.data, out.proj.ctypes.data,
                                                  out.edge.ctypes.data, out.info.ctypes.data))
        out.info = out.info[0]
        return out

    def kmeans_device(self, tree, branch_length, num_clusters: int, max_iterations: int, d_samples: int, d_clusters: int,
                      d_centroids: int, d_info: int, stream: int = 0) -> None:
        """The phylogenetic k-means into device memory: d_samples `capi.KMEANS_SAMPLE` [S], d_clusters
        `capi.KMEANS_CLUSTER` [K], d_centroids float64 [K][N], d_info one `capi.KMEANS_INFO`, every cell written.
        Synchronises `stream` once per iteration (`epik_amd_cohort_kmeans_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_kmeans_device(self._handle, tree._handle, length.ctypes.data,
                                                           _count32(num_clusters, "num_clusters"),
                                                           _count32(max_iterations, "max_iterations"), d_samples or None,
                                                           d_clusters or None, d_centroids or None, d_info or None, stream or None))

    def kmeans(self, tree, branch_length, num_clusters: int, max_iterations: int = 100) -> Kmeans:
        """The phylogenetic k-means of the samples, a `Kmeans` (`epik_amd_cohort_kmeans`)."""
        length = self._lengths(tree, branch_length)
        k, m = _count32(num_clusters, "num_clusters"), _count32(max_iterations, "max_iterations")
        out = _kmeans_buffers(self.num_samples, self.num_branches, k)
        capi.check(self._lib.epik_amd_cohort_kmeans(self._handle, tree._handle, length.ctypes.data, k, m, out.samples.ctypes.data,
                                                    out.clusters.ctypes.data, out.centroids.ctypes.data, out.info.ctypes.data))
        out.info = out.info[0]
        return out

    def alpha_device(self, tree, branch_length, d_alpha: int, stream: int = 0) -> None:
        """The alpha diversity indices into d_alpha, `capi.ALPHA` [S] in device memory, every cell written; asynchronous
        on `stream` once the lengths (host) are copied, no readback (`epik_amd_cohort_alpha_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_alpha_device(self._handle, tree._handle, length.ctypes.data, d_alpha or None,
                                                          stream or None))

    def alpha(self, tree, branch_length) -> np.ndarray:
        """The alpha diversity indices of the samples, `capi.ALPHA` [S] (`epik_amd_cohort_alpha`)."""
        length = self._lengths(tree, branch_length)
        out = np.full(self.num_samples * 5, np.nan).view(capi.ALPHA)
        capi.check(self._lib.epik_amd_cohort_alpha(self._handle, tree._handle, length.ctypes.data, out.ctypes.data))
        return out

    def rarefy_device(self, tree, branch_length, depth_step: int, num_depths: int, d_curve: int, stream: int = 0) -> None:
        """The rarefaction curves into d_curve, float64 [S][J][2] in device memory, every cell written; asynchronous on
        `stream` once the lengths (host) are copied, no readback (`epik_amd_cohort_rarefy_device`)."""
        length = self._lengths(tree, branch_length)
        capi.check(self._lib.epik_amd_cohort_rarefy_device(self._handle, tree._handle, length.ctypes.data,
                                                           _count32(depth_step, "depth_step"), _count32(num_depths, "num_depths"),
                                                           d_curve or None, stream or None))

    def rarefy(self, tree, branch_length, depth_step: int, num_depths: int) -> np.ndarray:
        """The rarefaction curves of the samples, float64 [S][J][2] (`epik_amd_cohort_rarefy`)."""
        length = self._lengths(tree, branch_length)
        step, depths = _count32(depth_step, "depth_step"), _count32(num_depths, "num_depths")
        out = _curve_buffer(self.num_samples, depths)
        capi.check(self._lib.epik_amd_cohort_rarefy(self._handle, tree._handle, length.ctypes.data, step, depths, out.ctypes.data))
        return out

    @staticmethod
    def _tree_handle(tree, what):
        if tree is None or not getattr(tree, "_handle", None):
            raise ValueError(f"{what} needs a device tree (Placer.tree)")
        return tree._handle

    def correlation_device(self, tree, meta, d_out: int, d_used: int, stream: int = 0) -> None:
        """The edge correlation with meta[S][M] (host; NaN: missing) into d_out, `capi.CORRELATION` [M][N], and d_used,
        uint32 [M], in device memory, every cell written; asynchronous on `stream` once the columns are copied, no readback
        (`epik_amd_cohort_correlation_device`)."""
        meta = _metadata(meta, self.num_samples)
        capi.check(self._lib.epik_amd_cohort_correlation_device(self._handle, self._tree_handle(tree, "correlation"),
                                                                meta.ctypes.data, meta.shape[1], d_out or None, d_used or None,
                                                                stream or None))

    def correlation(self, tree, meta):
        """The edge correlation of the samples with meta[S][M]: (`capi.CORRELATION` [M][N], used uint32 [M])
        (`epik_amd_cohort_correlation`)."""
        meta = _metadata(meta, self.num_samples)
        m, n = meta.shape[1], self.num_branches
        out, used = _na(max(m, 1) * n, capi.CORRELATION), np.zeros(max(m, 1), dtype=np.uint32)
        capi.check(self._lib.epik_amd_cohort_correlation(self._handle, self._tree_handle(tree, "correlation"), meta.ctypes.data, m,
                                                         out.ctypes.data, used.ctypes.data))
        return out.reshape(max(m, 1), n), used

    def dispersion_device(self, tree, d_out: int, stream: int = 0) -> None:
        """The edge dispersion into d_out, `capi.DISPERSION` [N] in device memory, every cell written; asynchronous on
        `stream`, no readback (`epik_amd_cohort_dispersion_device`)."""
        capi.check(self._lib.epik_amd_cohort_dispersion_device(self._handle, self._tree_handle(tree, "dispersion"), d_out or None,
                                                               stream or None))

    def dispersion(self, tree) -> np.ndarray:
        """The edge dispersion of the samples, `capi.DISPERSION` [N] (`epik_amd_cohort_dispersion`)."""
        out = _na(self.num_branches, capi.DISPERSION)
        capi.check(self._lib.epik_amd_cohort_dispersion(self._handle, self._tree_handle(tree, "dispersion"), out.ctypes.data))
        return out

    def permanova_device(self, d_kr: int, labels, permutations: int, seed: int, pairwise: bool, d_out: int, d_ssw: int = 0,
                         d_group_ss: int = 0, stream: int = 0, strata=None) -> None:
        """PERMANOVA of labels[S][M] (host; 0xffffffff: missing) over d_kr, float64 [S][S] in device memory as `kr_device`
        wrote it, into d_out, `capi.PERMANOVA` [M][1 + Q], and where given d_ssw, float64 [M][1 + Q][P + 1], and
        d_group_ss, float64 [M][256], every cell written; asynchronous on `stream` once the labels are copied, no readback
        (`epik_amd_cohort_permanova_device`)."""
        labels = _labels(labels, self.num_samples)
        _call(self._lib, "permanova_device", strata, self.num_samples, self._handle, d_kr or None, labels.ctypes.data, labels.shape[1],
              int(permutations), int(seed), int(bool(pairwise)), d_out or None,
              d_ssw or None, d_group_ss or None, stream or None)

    def permanova(self, tree, branch_length, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                  with_ssw: bool = False, metric="kr", strata=None) -> Permanova:
        """PERMANOVA of the samples' groups in every column of labels[S][M] over their distances `metric`, KR by default
        (`epik_amd_cohort_permanova_metric`).  `strata`, one id per sample: the shuffles stay within the strata
        (`epik_amd_cohort_permanova_strata`); likewise for `permdisp`, `edgetest`, `model` and the `_device` forms."""
        length = self._lengths(tree, branch_length)
        labels = _labels(labels, self.num_samples)
        records, ssw, group_ss = _permanova_buffers(labels.shape[1], permutations, pairwise, with_ssw)
        _call(self._lib, "permanova_metric", strata, self.num_samples, self._handle, tree._handle, length.ctypes.data,
              metric_id(metric), labels.ctypes.data, labels.shape[1], int(permutations), int(seed),
              int(bool(pairwise)), records.ctypes.data,
              ssw.ctypes.data if with_ssw else None, group_ss.ctypes.data)
        return Permanova(records, ssw, group_ss)

    def permdisp_device(self, d_kr: int, labels, permutations: int, seed: int, pairwise: bool, d_out: int, d_group_mean: int,
                        d_z: int, d_stat: int = 0, stream: int = 0, strata=None) -> None:
        """PERMDISP of labels[S][M] (host; 0xffffffff: missing) over d_kr, float64 [S][S] in device memory as `kr_device`
        wrote it, into d_out, `capi.PERMDISP` [M][1 + Q], d_group_mean, float64 [M][32], d_z, float64 [M][S], and where given
        d_stat, float64 [M][1 + Q][P + 1], every cell written; asynchronous on `stream` once the labels are copied, no
        readback (`epik_amd_cohort_permdisp_device`)."""
        labels = _labels(labels, self.num_samples)
        _call(self._lib, "permdisp_device", strata, self.num_samples, self._handle, d_kr or None, labels.ctypes.data, labels.shape[1],
              int(permutations), int(seed), int(bool(pairwise)), d_out or None,
              d_stat or None, d_group_mean or None, d_z or None, stream or None)

    def permdisp(self, tree, branch_length, labels, permutations: int = 999, seed: int = 1, pairwise: bool = False,
                 with_stat: bool = False, metric="kr", strata=None) -> Permdisp:
        """PERMDISP of the samples' groups in every column of labels[S][M]: do they differ in their distances to the group
        centroids over the distances `metric`, KR by default (`epik_amd_cohort_permdisp_metric`)."""
        length = self._lengths(tree, branch_length)
        labels = _labels(labels, self.num_samples)
        out = _permdisp_buffers(labels.shape[1], self.num_samples, permutations, pairwise, with_stat)
        _call(self._lib, "permdisp_metric", strata, self.num_samples, self._handle, tree._handle, length.ctypes.data,
              metric_id(metric), labels.ctypes.data, labels.shape[1], int(permutations), int(seed),
              int(bool(pairwise)), out.records.ctypes.data,
              out.stat.ctypes.data if with_stat else None, out.group_mean.ctypes.data,
              out.z.ctypes.data)
        return out

    def mantel_device(self, d_dist: int, values=None, matrices=None, matrix_present=None, methods=("pearson",), control=None,
                      permutations: int = 999, seed: int = 1, d_out: int = 0, d_stat: int = 0, stream: int = 0, strata=None) -> None:
        """The Mantel tests of the sides (host; `mantel`) over d_dist, float64 [S][S] in device memory as `kr_device` or
        `unifrac_device` wrote it, into d_out, `capi.MANTEL` [tests], and where given d_stat, float64 [tests][P + 1], every cell
        written; asynchronous on `stream` once the sides are copied, no readback (`epik_amd_cohort_mantel_device`)."""
        keep, args, _ = _sides(values, matrices, matrix_present, methods, control, permutations, self.num_samples, False)
        strata = _strata(strata, self.num_samples)
        capi.check(self._lib.epik_amd_cohort_mantel_device(self._handle, d_dist or None, *args, int(seed), _pointer(strata),
                                                           d_out or None, d_stat or None, stream or None))

    def mantel(self, tree, branch_length, values=None, matrices=None, matrix_present=None, methods=("pearson",), control=None,
               permutations: int = 999, seed: int = 1, metric="kr", strata=None, with_stat: bool = False) -> Mantel:
        """The Mantel test of every side against the samples' distances `metric`, KR by default: values [Mv][S], a column of
        numbers a side (NaN: missing; its distance is |v_s - v_t|), and matrices [Mm][S][S] with matrix_present [Mm][S].
        `methods`: pearson, spearman or both; `control`: the side held fixed (the partial Mantel test of every other side);
        `strata`, one id per sample: the shuffles stay within the strata (`epik_amd_cohort_mantel`)."""
        length = self._lengths(tree, branch_length)
        keep, args, out = _sides(values, matrices, matrix_present, methods, control, permutations, self.num_samples, with_stat)
        strata = _strata(strata, self.num_samples)
        capi.check(self._lib.epik_amd_cohort_mantel(self._handle, tree._handle, length.ctypes.data, metric_id(metric), *args, int(seed),
                                                    _pointer(strata), out.records.ctypes.data, _pointer(out.stat)))
        return out

    def anosim_device(self, d_dist: int, labels, permutations: int, seed: int, d_out: int, d_stat: int = 0, stream: int = 0,
                      strata=None) -> None:
        """ANOSIM of labels[S][M] (host; 0xffffffff: missing) over d_dist as `mantel_device` takes it, into d_out, `capi.ANOSIM`
        [M], and where given d_stat, float64 [M][P + 1], every cell written; asynchronous on `stream` once the labels are copied,
        no readback (`epik_amd_cohort_anosim_device`)."""
        labels = _labels(labels, self.num_samples)
        strata = _strata(strata, self.num_samples)
        capi.check(self._lib.epik_amd_cohort_anosim_device(self._handle, d_dist or None, labels.ctypes.data, labels.shape[1],
                                                           int(permutations), int(seed), _pointer(strata), d_out or None,
                                                           d_stat or None, stream or None))

    def anosim(self, tree, branch_length, labels, permutations: int = 999, seed: int = 1, metric="kr", strata=None,
               with_stat: bool = False) -> Anosim:
        """ANOSIM of the samples' groups in every column of labels[S][M] over the ranks of their distances `metric`, KR by
        default (`epik_amd_cohort_anosim`)."""
        length = self._lengths(tree, branch_length)
        labels = _labels(labels, self.num_samples)
        out = _anosim_buffers(labels.shape[1], permutations, with_stat)
        strata = _strata(strata, self.num_samples)
        capi.check(self._lib.epik_amd_cohort_anosim(self._handle, tree._handle, length.ctypes.data, metric_id(metric),
                                                    labels.ctypes.data, labels.shape[1], int(permutations), int(seed),
                                                    _pointer(strata), out.records.ctypes.data, _pointer(out.stat)))
        return out

    def pcoa_device(self, d_kr: int, num_components: int, d_mu: int, d_coord: int, d_info: int, stream: int = 0) -> None:
        """The principal coordinates over d_kr, float64 [S][S] in device memory as `kr_device` wrote it, into device memory:
        d_mu float64 [S], d_coord float64 [S][K], d_info one `capi.PCOA_INFO`, every cell written.  Synchronises `stream`
        once for the number of used samples and, on the eigensolver's global path, once per sweep
        (`epik_amd_cohort_pcoa_device`)."""
        capi.check(self._lib.epik_amd_cohort_pcoa_device(self._handle, d_kr or None, _components(num_components), d_mu or None,
                                                         d_coord or None, d_info or None, stream or None))

    def pcoa(self, tree, branch_length, num_components: int = 5, metric="kr") -> Pcoa:
        """The principal coordinates of the samples over their distances `metric`, KR by default, a `Pcoa`
        (`epik_amd_cohort_pcoa_metric`)."""
        length = self._lengths(tree, branch_length)
        k = _components(num_components)
        out = _pcoa_buffers(self.num_samples, k)
        capi.check(self._lib.epik_amd_cohort_pcoa_metric(self._handle, tree._handle, length.ctypes.data, metric_id(metric), k,
                                                         out.mu.ctypes.data, out.coord.ctypes.data, out.info.ctypes.data))
        out.info = out.info[0]
        return out

    def edgetest_device(self, tree, labels, permutations: int, seed: int, d_out: int, d_stat: int = 0, d_max: int = 0,
                        stream: int = 0, strata=None) -> None:
        """The edge test of labels[S][M] (host; 0xffffffff: missing) into d_out, `capi.EDGETEST` [M][N], and where given
        d_stat, float64 [M][4][N][P + 1], and d_max, float64 [M][4][P + 1], all in device memory, every cell written;
        asynchronous on `stream` once the labels are copied, no readback (`epik_amd_cohort_edgetest_device`)."""
        labels = _labels(labels, self.num_samples)
        _call(self._lib, "edgetest_device", strata, self.num_samples, self._handle, self._tree_handle(tree, "edgetest_device"),
              labels.ctypes.data, labels.shape[1], int(permutations), int(seed),
              d_out or None, d_stat or None, d_max or None, stream or None)

    def edgetest(self, tree, labels, permutations: int = 999, seed: int = 1, with_stat: bool = False,
                 with_max: bool = False, strata=None) -> Edgetest:
        """Which branches differ between the groups of every column of labels[S][M]: per branch the one-way ANOVA and
        Kruskal-Wallis of its mass and imbalance by permutation, with the max-statistic adjustment
        (`epik_amd_cohort_edgetest`)."""
        labels = _labels(labels, self.num_samples)
        records, stat, most = _edgetest_buffers(labels.shape[1], self.num_branches, permutations, with_stat, with_max)
        _call(self._lib, "edgetest", strata, self.num_samples, self._handle, self._tree_handle(tree, "edgetest"), labels.ctypes.data,
              labels.shape[1], int(permutations), int(seed), records.ctypes.data,
              stat.ctypes.data if with_stat else None,
              most.ctypes.data if with_max else None)
        return Edgetest(records, stat, most)

    def model_device(self, d_kr: int, kind, labels, values, permutations: int, seed: int, d_out: int, d_info: int, d_aliased: int,
                     d_stat: int = 0, stream: int = 0, strata=None) -> None:
        """The sequential model of the design kind[T], labels[S][T] and values[S][T] (host) over d_kr, float64 [S][S] in
        device memory as `kr_device` wrote it, into d_out, `capi.MODEL_TERM` [T + 1], d_info, one `capi.MODEL_INFO`, d_aliased,
        64 bytes, and where given d_stat, float64 [T + 1][P + 1], every cell written; asynchronous on `stream` once the design
        is copied, no readback (`epik_amd_cohort_model_device`)."""
        kind, labels, values = _design(kind, labels, values, self.num_samples)
        _call(self._lib, "model_device", strata, self.num_samples, self._handle, d_kr or None, kind.ctypes.data, labels.ctypes.data,
              values.ctypes.data, kind.shape[0], int(permutations), int(seed),
              d_out or None, d_info or None, d_stat or None, d_aliased or None,
              stream or None)

    def model(self, tree, branch_length, kind, labels, values, permutations: int = 999, seed: int = 1, with_stat: bool = False,
              metric="kr", strata=None) -> Model:
        """The sequential model of the samples over their distances `metric`, KR by default: every term of the design tested
        after the terms before it (`epik_amd_cohort_model_metric`)."""
        length = self._lengths(tree, branch_length)
        kind, labels, values = _design(kind, labels, values, self.num_samples)
        records, info, stat, aliased = _model_buffers(kind.shape[0], permutations, with_stat)
        _call(self._lib, "model_metric", strata, self.num_samples, self._handle, tree._handle, length.ctypes.data, metric_id(metric),
              kind.ctypes.data, labels.ctypes.data, values.ctypes.data, kind.shape[0],
              int(permutations), int(seed), records.ctypes.data, info.ctypes.data,
              stat.ctypes.data if with_stat else None, aliased.ctypes.data)
        return Model(records, info[0], stat, aliased)

    def edgemodel_device(self, tree, kind, labels, values, permutations: int, seed: int, d_out: int, d_info: int, d_aliased: int,
                         d_stat: int = 0, d_max: int = 0, stream: int = 0, strata=None) -> None:
        """The edge model of the design kind[T], labels[S][T] and values[S][T] (host) into d_out, `capi.EDGEMODEL` [T][N],
        d_info, one `capi.EDGEMODEL_INFO`, d_aliased, 64 bytes, and where given d_stat, float64 [T][2][N][P + 1], and d_max,
        float64 [T][2][P + 1], all in device memory, every cell written; asynchronous on `stream` once the design is copied,
        no readback (`epik_amd_cohort_edgemodel_device`)."""
        kind, labels, values = _design(kind, labels, values, self.num_samples)
        _call(self._lib, "edgemodel_device", strata, self.num_samples, self._handle, self._tree_handle(tree, "edgemodel_device"),
              kind.ctypes.data, labels.ctypes.data, values.ctypes.data, kind.shape[0], int(permutations), int(seed),
              d_out or None, d_info or None, d_stat or None, d_max or None, d_aliased or None, stream or None)

    def edgemodel(self, tree, kind, labels, values, permutations: int = 999, seed: int = 1, with_stat: bool = False,
                  with_max: bool = False, strata=None) -> Edgemodel:
        """On which branches a term of the design still matters after the terms before it: per branch the sequential linear
        model of its mass and imbalance by permutation, with the max-statistic adjustment (`epik_amd_cohort_edgemodel`)."""
        kind, labels, values = _design(kind, labels, values, self.num_samples)
        records, info, stat, most, aliased = _edgemodel_buffers(kind.shape[0], self.num_branches, permutations, with_stat, with_max)
        _call(self._lib, "edgemodel", strata, self.num_samples, self._handle, self._tree_handle(tree, "edgemodel"), kind.ctypes.data,
              labels.ctypes.data, values.ctypes.data, kind.shape[0], int(permutations), int(seed), records.ctypes.data,
              info.ctypes.data, stat.ctypes.data if with_stat else None, most.ctypes.data if with_max else None,
              aliased.ctypes.data)
        return Edgemodel(records, info[0], stat, most, aliased)

    def reset(self) -> None:
        capi.check(self._lib.epik_amd_cohort_reset(self._handle))


# ---- the files of --cohort -------------------------------------------------------------------------------------------
def format_samples_tsv(names, cells: CohortCells) -> str:
    lines = [SAMPLES_HEADER]
    records = cells.records()
    for s, name in enumerate(names):
        t = cells.totals[s]
        total_mass = int(cells.mass[s].sum(dtype=np.uint64))
        lines.append(f"{name}\t{int(records[s])}\t{int(t['placed'])}\t{int(t['no_hit'])}\t{int(t['too_short'])}"
                     f"\t{int(t['too_narrow'])}\t{total_mass}")
    return "\n".join(lines) + "\n"


def format_profile_tsv(names, cells: CohortCells) -> str:
    lines = [PROFILE_HEADER]
    for s, name in enumerate(names):
        for b in np.flatnonzero((cells.mass[s] != 0) | (cells.best[s] != 0)):
            lines.append(f"{name}\t{int(b)}\t{int(cells.best[s, b])}\t{int(cells.mass[s, b])}")
    return "\n".join(lines) + "\n"


def format_kr_tsv(names, kr) -> str:
    lines = ["\t".join(["name", *names])]
    for s, name in enumerate(names):
        lines.append("\t".join([name, *("%.17g" % float(x) for x in kr[s])]))
    return "\n".join(lines) + "\n"


def format_unifrac_tsv(names, matrix) -> str:
    """cohort_unifrac_<metric>_<list>.tsv: the square layout of `format_kr_tsv`, doubles as %.17g."""
    return format_kr_tsv(names, matrix)


def _distance_field(distance) -> str:
    """What the first line of a PCoA, PERMANOVA or PERMDISP file ends in: nothing over KR, else <TAB>distance=NAME."""
    name = DISTANCES[metric_id(distance)] if not isinstance(distance, str) else distance
    if name not in DISTANCES:
        raise ValueError(f"unknown distance {name!r} (one of {', '.join(DISTANCES)})")
    return "" if name == "kr" else f"\tdistance={name}"


_DISTANCE_FIELD = r"(?:\tdistance=(unweighted|weighted|generalized))?"
_STRATA_FIELD = r"(?:\tstrata=(?P<strata>[^\t]+))?"  # the last field of the first line of the four permutation tests' files


def _live_mask(names, live) -> np.ndarray:
    live = np.asarray(live, dtype=bool)
    if live.shape != (len(names),):
        raise ValueError(f"live must hold one flag per sample ({len(names)})")
    return live


def format_squash_tsv(names, live, merges) -> str:
    """cohort_squash_<list>.tsv: `live[s]`: sample s has mass (T_s > 0) and is clustered; `merges` the records made."""
    live = _live_mask(names, live)
    s = len(names)
    lines = [f"# epik_amd squash v1  samples={s} clustered={int(live.sum())} merges={len(merges)}"]
    lines += [f"# unclustered\t{name}" for name, alive in zip(names, live) if not alive]
    lines.append(SQUASH_HEADER)
    size = [1] * s
    for t, m in enumerate(merges):
        size.append(size[int(m["a"])] + size[int(m["b"])])
        lines.append("\t".join([str(t), str(s + t), str(int(m["a"])), str(int(m["b"])), str(size[-1]),
                                *("%.17g" % float(m[k]) for k in ("dist", "len_a", "len_b"))]))
    return "\n".join(lines) + "\n"


def newick_label(name: str) -> str:
    """The name as it is when all of [A-Za-z0-9_.-], else in single quotes with the inner quotes doubled."""
    return name if re.fullmatch(r"[A-Za-z0-9_.-]+", name) else "'" + name.replace("'", "''") + "'"


def format_squash_newick(names, live, merges) -> str:
    """cohort_squash_<list>.nwk: the cluster tree, child a before child b, no length at the root; `name;` for one
    clustered sample, `;` for none."""
    live = _live_mask(names, live)
    text = [newick_label(name) if alive else "" for name, alive in zip(names, live)]
    for m in merges:        # (bottom up: a record names only nodes made before it)
        text.append("(%s:%.17g,%s:%.17g)" % (text[int(m["a"])], float(m["len_a"]), text[int(m["b"])], float(m["len_b"])))
    if len(merges):
        return text[-1] + ";\n"
    return (text[int(np.flatnonzero(live)[0])] if live.any() else "") + ";\n"


def read_squash_tsv(path: str):
    """(merges, info): the records, `capi.SQUASH_MERGE` [M], and {"samples", "clustered", "merges", "unclustered": names,
    "node", "size": arrays [M]}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd squash v1  samples=(\d+) clustered=(\d+) merges=(\d+)", fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort squash file")
        info = {"samples": int(head[1]), "clustered": int(head[2]), "merges": int(head[3]), "unclustered": []}
        line = fh.readline().rstrip("\n")
        while line.startswith("# unclustered\t"):
            info["unclustered"].append(line.split("\t", 1)[1])
            line = fh.readline().rstrip("\n")
        if line != SQUASH_HEADER:
            raise ValueError(f"{path}: not a cohort squash file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if len(rows) != info["merges"] or [int(r[0]) for r in rows] != list(range(len(rows))):
        raise ValueError(f"{path}: the steps do not follow the first line's count")
    merges = np.zeros(len(rows), dtype=capi.SQUASH_MERGE)
    for t, r in enumerate(rows):
        merges[t] = (int(r[2]), int(r[3]), float(r[5]), float(r[6]), float(r[7]))
    info["node"] = np.array([int(r[1]) for r in rows], dtype=np.int64)
    info["size"] = np.array([int(r[4]) for r in rows], dtype=np.int64)
    return merges, info


# ---- the files of --cohort-epca ----------------------------------------------------------------------------------------
def _epca_columns(k: int) -> str:
    return "".join(f"\tpc{i + 1}" for i in range(k))


def format_epca_tsv(names, used, epca: Epca) -> str:
    """cohort_epca_<list>.tsv (`used[s]`: sample s has mass, T_s > 0): the first line, a `# unused` line per sample without mass, a `# component` line per
    component (k from 1; mu, lambda = mu / max(L - 1, 1), fraction = mu / trace or 0; null|ok), the column names, then
    per used sample, in list order, its name and its projections; doubles as %.17g."""
    info = epca.info
    is_used = _live_mask(names, used)
    used, kc = int(info["used"]), int(info["components"])
    s = len(names)
    if int(is_used.sum()) != used:
        raise ValueError("the used flags do not fit the number of used samples")
    lines = [f"# epik_amd epca v1  samples={s} used={used} components={kc} sweeps={int(info['sweeps'])} "
             f"converged={int(info['converged'])}"]
    lines += [f"# unused\t{name}" for name, u in zip(names, is_used) if not u]
    trace, null = float(info["trace"]), epca.null()
    for k in range(kc):
        mu = float(epca.mu[k])
        lam, fraction = mu / float(max(used - 1, 1)), (mu / trace if trace != 0 else 0.0)
        lines.append("# component\t%d\t%.17g\t%.17g\t%.17g\t%s" % (k + 1, mu, lam, fraction, "null" if null[k] else "ok"))
    lines.append("name" + _epca_columns(kc))
    for i, name in enumerate(names):
        if is_used[i]:
            lines.append("\t".join([name, *("%.17g" % float(x) for x in epca.proj[i, :kc])]))
    return "\n".join(lines) + "\n"


def format_epca_edges_tsv(first, epca: Epca) -> str:
    """cohort_epca_edges_<list>.tsv: edge_num and the components' coefficients for every inner branch (first[b] < b) in id
    order; doubles as %.17g."""
    kc = int(epca.info["components"])
    first = np.asarray(first, dtype=np.int64)
    lines = ["edge_num" + _epca_columns(kc)]
    for b in np.flatnonzero(first < np.arange(len(first))):
        lines.append("\t".join([str(int(b)), *("%.17g" % float(x) for x in epca.edge[:kc, b])]))
    return "\n".join(lines) + "\n"


def read_epca_tsv(path: str):
    """(names, proj, info): the used samples' names, float64 [L][K'], and {"samples", "used", "components", "sweeps",
    "converged", "unused": names, "mu", "lambda", "fraction": float64 [K'], "null": bool [K']}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd epca v1  samples=(\d+) used=(\d+) components=(\d+) sweeps=(\d+) converged=([01])",
                            fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort epca file")
        info = dict(zip(("samples", "used", "components", "sweeps", "converged"), (int(x) for x in head.groups())))
        info["unused"] = []
        comps = []
        line = fh.readline().rstrip("\n")
        while line.startswith("# "):
            kind, rest = line[2:].split("\t", 1)
            if kind == "unused":
                info["unused"].append(rest)
            elif kind == "component":
                comps.append(rest.split("\t"))
            else:
                raise ValueError(f"{path}: not a cohort epca file")
            line = fh.readline().rstrip("\n")
        kc = info["components"]
        if line != "name" + _epca_columns(kc) or [int(c[0]) for c in comps] != list(range(1, kc + 1)):
            raise ValueError(f"{path}: the components do not follow the first line's count")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if len(rows) != info["used"] or any(len(r) != kc + 1 for r in rows):
        raise ValueError(f"{path}: the rows do not follow the first line's counts")
    info["mu"] = np.array([float(c[1]) for c in comps], dtype=np.float64)
    info["lambda"] = np.array([float(c[2]) for c in comps], dtype=np.float64)
    info["fraction"] = np.array([float(c[3]) for c in comps], dtype=np.float64)
    info["null"] = np.array([c[4] == "null" for c in comps], dtype=bool)
    proj = np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(rows), kc)
    return [r[0] for r in rows], proj, info


def read_epca_edges_tsv(path: str):
    """(edge_num int64 [E], coefficients float64 [E][K'])"""
    with open(path, newline="") as fh:
        head = fh.readline().rstrip("\n").split("\t")
        if head[0] != "edge_num" or head[1:] != [f"pc{i + 1}" for i in range(len(head) - 1)]:
            raise ValueError(f"{path}: not a cohort epca edges file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    kc = len(head) - 1
    return (np.array([int(r[0]) for r in rows], dtype=np.int64),
            np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(rows), kc))


# ---- the files of --cohort-kmeans --------------------------------------------------------------------------------------
# ---- the file of --cohort-pcoa ------------------------------------------------------------------------------------------
def format_pcoa_tsv(names, totals, pcoa: Pcoa, distance="kr") -> str:
    """cohort_pcoa_<list>.tsv (`totals[s]`: T_s, only > 0 matters): the first line with negative = -neg / pos, a `# unused`
    line per sample without mass, a `# eigenvalue` line for each of the L eigenvalues (k from 1; mu, fraction = mu / pos or
    0; real|null|negative), the column names, then per used sample, in list order, its name and its coordinates; doubles
    as %.17g.  Over a `distance` other than KR the first line ends in <TAB>distance=NAME."""
    info = pcoa.info
    is_used = np.asarray(totals) != 0
    used, kc = int(info["used"]), int(info["components"])
    if len(is_used) != len(names) or int(is_used.sum()) != used:
        raise ValueError("the totals do not fit the number of used samples")
    lines = [f"# epik_amd pcoa v1  samples={len(names)} used={used} components={kc} sweeps={int(info['sweeps'])} "
             f"converged={int(info['converged'])} negative={'%.17g' % pcoa.negative}" + _distance_field(distance)]
    lines += [f"# unused\t{name}" for name, u in zip(names, is_used) if not u]
    pos = float(info["pos"])
    for k, kind in enumerate(pcoa.kinds()):
        mu = float(pcoa.mu[k])
        lines.append("# eigenvalue\t%d\t%.17g\t%.17g\t%s" % (k + 1, mu, mu / pos if pos != 0 else 0.0, kind))
    lines.append("name" + _epca_columns(kc))
    for i, name in enumerate(names):
        if is_used[i]:
            lines.append("\t".join([name, *("%.17g" % float(x) for x in pcoa.coord[i, :kc])]))
    return "\n".join(lines) + "\n"


def read_pcoa_tsv(path: str):
    """(names, coord, info): the used samples' names, float64 [L][K'], and {"samples", "used", "components", "sweeps",
    "converged", "negative", "unused": names, "mu", "fraction": float64 [L], "kind": the classes; and "distance", a name of
    `DISTANCES`, only where the first line has the field: a file over KR has none}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd pcoa v1  samples=(\d+) used=(\d+) components=(\d+) sweeps=(\d+) converged=([01]) "
                            r"negative=([^\s]+)" + _DISTANCE_FIELD, fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort pcoa file")
        info = dict(zip(("samples", "used", "components", "sweeps", "converged"), map(int, head.groups()[:5])))
        info["negative"] = float(head.group(6))
        if head.group(7):                     # (a file over KR has no such field, and its info no such key)
            info["distance"] = head.group(7)
        unused, eig, line = [], [], fh.readline().rstrip("\n")
        while line.startswith("# "):
            fields = line.split("\t")
            if fields[0] == "# unused" and len(fields) == 2:
                unused.append(fields[1])
            elif fields[0] == "# eigenvalue" and len(fields) == 5:
                eig.append(fields[1:])
            else:
                raise ValueError(f"{path}: not a cohort pcoa file")
            line = fh.readline().rstrip("\n")
        kc = info["components"]
        if line != "name" + _epca_columns(kc) or [int(e[0]) for e in eig] != list(range(1, info["used"] + 1)):
            raise ValueError(f"{path}: the eigenvalues or the column names do not fit the first line")
        rows = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()]
    if len(rows) != info["used"] or any(len(r) != kc + 1 for r in rows):
        raise ValueError(f"{path}: the rows do not fit the first line")
    info.update(unused=unused, mu=np.array([float(e[1]) for e in eig]), fraction=np.array([float(e[2]) for e in eig]),
                kind=[e[3] for e in eig])
    coord = np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(rows), kc)
    return [r[0] for r in rows], coord, info


def format_kmeans_tsv(names, kmeans: Kmeans) -> str:
    """cohort_kmeans_<list>.tsv: the first line, a `# unused` line per sample without mass, a `# cluster` line per cluster
    k < K' (k, size, the seed's name, sum_dist, sum_sq), the column names, then per used sample, in list order, its name,
    cluster and dist; doubles as %.17g."""
    info, samples = kmeans.info, kmeans.samples
    if len(samples) != len(names):
        raise ValueError("one record per sample")
    used = samples["cluster"] != capi.KMEANS_NONE
    if int(used.sum()) != int(info["used"]):
        raise ValueError("the records do not fit the number of used samples")
    lines = [f"# epik_amd kmeans v1  samples={len(names)} used={int(info['used'])} clusters={int(info['clusters'])} "
             f"iterations={int(info['iterations'])} converged={int(info['converged'])}"]
    lines += [f"# unused\t{name}" for name, u in zip(names, used) if not u]
    for k in range(int(info["clusters"])):
        c = kmeans.clusters[k]
        lines.append("# cluster\t%d\t%d\t%s\t%.17g\t%.17g" % (k, int(c["size"]), names[int(c["seed"])], float(c["sum_dist"]),
                                                              float(c["sum_sq"])))
    lines.append("name\tcluster\tdist")
    for i, name in enumerate(names):
        if used[i]:
            lines.append("%s\t%d\t%.17g" % (name, int(samples["cluster"][i]), float(samples["dist"][i])))
    return "\n".join(lines) + "\n"


def format_kmeans_centroids_tsv(kmeans: Kmeans) -> str:
    """cohort_kmeans_centroids_<list>.tsv: cluster, edge_num and mass for every non-zero cell of the centroids of the
    clusters k < K'; doubles as %.17g."""
    lines = ["cluster\tedge_num\tmass"]
    for k in range(int(kmeans.info["clusters"])):
        row = kmeans.centroids[k]
        lines += ["%d\t%d\t%.17g" % (k, int(b), float(row[b])) for b in np.flatnonzero(row != 0)]
    return "\n".join(lines) + "\n"


def read_kmeans_tsv(path: str):
    """(names, cluster int64 [L], dist float64 [L], info): the used samples in list order, and {"samples", "used",
    "clusters", "iterations", "converged", "unused": names, "size": int64 [K'], "seed": names, "sum_dist", "sum_sq":
    float64 [K']}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd kmeans v1  samples=(\d+) used=(\d+) clusters=(\d+) iterations=(\d+) converged=([01])",
                            fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort kmeans file")
        info = dict(zip(("samples", "used", "clusters", "iterations", "converged"), (int(x) for x in head.groups())))
        info["unused"] = []
        clusters = []
        line = fh.readline().rstrip("\n")
        while line.startswith("# "):
            kind, rest = line[2:].split("\t", 1)
            if kind == "unused":
                info["unused"].append(rest)
            elif kind == "cluster":
                clusters.append(rest.split("\t"))
            else:
                raise ValueError(f"{path}: not a cohort kmeans file")
            line = fh.readline().rstrip("\n")
        if line != "name\tcluster\tdist" or [int(c[0]) for c in clusters] != list(range(info["clusters"])):
            raise ValueError(f"{path}: the clusters do not follow the first line's count")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if len(rows) != info["used"] or any(len(r) != 3 for r in rows) or any(len(c) != 5 for c in clusters):
        raise ValueError(f"{path}: the rows do not follow the first line's counts")
    info["size"] = np.array([int(c[1]) for c in clusters], dtype=np.int64)
    info["seed"] = [c[2] for c in clusters]
    info["sum_dist"] = np.array([float(c[3]) for c in clusters], dtype=np.float64)
    info["sum_sq"] = np.array([float(c[4]) for c in clusters], dtype=np.float64)
    return ([r[0] for r in rows], np.array([int(r[1]) for r in rows], dtype=np.int64),
            np.array([float(r[2]) for r in rows], dtype=np.float64), info)


def read_kmeans_centroids_tsv(path: str, num_clusters: int, num_branches: int) -> np.ndarray:
    """The centroids, float64 [num_clusters][num_branches], zero where the file has no line."""
    out = np.zeros((num_clusters, num_branches), dtype=np.float64)
    with open(path, newline="") as fh:
        if fh.readline().rstrip("\n") != "cluster\tedge_num\tmass":
            raise ValueError(f"{path}: not a cohort kmeans centroids file")
        for ln in fh:
            k, b, v = ln.rstrip("\n").split("\t")
            out[int(k), int(b)] = float(v)
    return out


ALPHA_HEADER = "name\tpd\trooted_pd\tbwpd_0.5\tbwpd_1\tquadratic_entropy"
RAREFY_HEADER = "name\tk\treads\tpd\trooted_pd"
_ALPHA_FIELDS = ("pd", "rooted_pd", "bwpd_half", "bwpd_one", "quadratic")


def format_alpha_tsv(names, alpha) -> str:
    """cohort_alpha_<list>.tsv: the first line, a `# unused` line per sample without mass (pd == -1), the column names,
    then per used sample, in list order, its name and the five indices; doubles as %.17g."""
    alpha = np.asarray(alpha)
    if alpha.dtype != capi.ALPHA or alpha.shape != (len(names),):
        raise ValueError("one capi.ALPHA record per sample")
    used = alpha["pd"] != -1.0
    lines = [f"# epik_amd alpha v1  samples={len(names)} used={int(used.sum())}"]
    lines += [f"# unused\t{name}" for name, u in zip(names, used) if not u]
    lines.append(ALPHA_HEADER)
    for i, name in enumerate(names):
        if used[i]:
            lines.append(name + "".join("\t%.17g" % float(alpha[f][i]) for f in _ALPHA_FIELDS))
    return "\n".join(lines) + "\n"


def read_alpha_tsv(path: str):
    """(names, alpha `capi.ALPHA` [L], info): the used samples in list order, and {"samples", "used", "unused": names}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd alpha v1  samples=(\d+) used=(\d+)", fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort alpha file")
        info = {"samples": int(head.group(1)), "used": int(head.group(2)), "unused": []}
        line = fh.readline().rstrip("\n")
        while line.startswith("# unused\t"):
            info["unused"].append(line.split("\t", 1)[1])
            line = fh.readline().rstrip("\n")
        if line != ALPHA_HEADER:
            raise ValueError(f"{path}: not a cohort alpha file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if len(rows) != info["used"] or any(len(r) != 6 for r in rows) or len(info["unused"]) != info["samples"] - info["used"]:
        raise ValueError(f"{path}: the rows do not follow the first line's counts")
    alpha = np.zeros(len(rows), dtype=capi.ALPHA)
    for i, r in enumerate(rows):
        alpha[i] = tuple(float(x) for x in r[1:])
    return [r[0] for r in rows], alpha, info


def reads_of(best) -> np.ndarray:
    """n_s of the rule: the wrapping sum of best[s][:], uint64 [S]."""
    return np.asarray(best, dtype=np.uint64).sum(axis=1, dtype=np.uint64)


def format_rarefy_tsv(names, reads, depth_step: int, curve) -> str:
    """cohort_rarefy_<list>.tsv: the first line, a `# unused` line per sample that is not rarefiable (`reads`[s] = n_s is 0
    or >= 2^53), the column names, then, long format, name, k, reads, pd and rooted_pd for every used sample and every
    k_j <= n_s of curve[S][J][2]; doubles as %.17g."""
    curve = np.asarray(curve, dtype=np.float64)
    reads = [int(x) for x in reads]
    step = int(depth_step)
    if curve.ndim != 3 or curve.shape[0] != len(names) or curve.shape[2] != 2 or len(reads) != len(names):
        raise ValueError("curve must be [num_samples][num_depths][2], with one read count per sample")
    used = [0 < n < (1 << 53) for n in reads]
    lines = [f"# epik_amd rarefy v1  samples={len(names)} used={sum(used)} step={step} depths={curve.shape[1]}"]
    lines += [f"# unused\t{name}" for name, u in zip(names, used) if not u]
    lines.append(RAREFY_HEADER)
    for i, name in enumerate(names):
        if used[i]:
            lines += ["%s\t%d\t%d\t%.17g\t%.17g" % (name, (j + 1) * step, reads[i], float(curve[i, j, 0]), float(curve[i, j, 1]))
                      for j in range(min(curve.shape[1], reads[i] // step))]
    return "\n".join(lines) + "\n"


def read_rarefy_tsv(path: str):
    """(rows, info): rows a list of (name, k, reads, pd, rooted_pd) in file order, and {"samples", "used", "step", "depths",
    "unused": names}."""
    with open(path, newline="") as fh:
        head = re.fullmatch(r"# epik_amd rarefy v1  samples=(\d+) used=(\d+) step=(\d+) depths=(\d+)", fh.readline().rstrip("\n"))
        if not head:
            raise ValueError(f"{path}: not a cohort rarefy file")
        info = dict(zip(("samples", "used", "step", "depths"), (int(x) for x in head.groups())))
        info["unused"] = []
        line = fh.readline().rstrip("\n")
        while line.startswith("# unused\t"):
            info["unused"].append(line.split("\t", 1)[1])
            line = fh.readline().rstrip("\n")
        if line != RAREFY_HEADER:
            raise ValueError(f"{path}: not a cohort rarefy file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if any(len(r) != 5 for r in rows) or len(info["unused"]) != info["samples"] - info["used"]:
        raise ValueError(f"{path}: the rows do not follow the first line's counts")
    return [(r[0], int(r[1]), int(r[2]), float(r[3]), float(r[4])) for r in rows], info


_NUMBER = re.compile(r"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?")


def read_metadata(path: str, names):
    """The metadata file of --cohort-correlation for the samples `names` of the list: (columns, float64 [S][M] in list order
    with NaN for a missing value, the number of lines skipped because their sample is not in the list).  A TSV: the header
    `sample<TAB>name1<TAB>...` (1 to 64 unique, non-empty names), then a line per sample; blank lines and `#` lines are
    skipped; a value is empty or `NA` (missing) or a decimal number.  ValueError naming the line, and the column where there
    is one, for anything else, and naming the sample of the list that the file lacks."""
    index = {name: s for s, name in enumerate(names)}
    columns, values, seen, skipped = None, None, {}, 0
    with open(path, newline="") as fh:
        for number, line in enumerate(fh, 1):
            line = line.rstrip("\n")
            if line.endswith("\r"):
                line = line[:-1]
            if not line or line.startswith("#"):
                continue
            where = f"{path} line {number}"
            fields = line.split("\t")
            if columns is None:
                if fields[0] != "sample":
                    raise ValueError(f"{where}: the header must begin with 'sample'")
                if not 2 <= len(fields) <= 1 + capi.CORRELATION_MAX_COLUMNS:
                    raise ValueError(f"{where}: the header names {len(fields) - 1} columns, not 1 to 64")
                columns = fields[1:]
                for c, name in enumerate(columns):
                    if not name:
                        raise ValueError(f"{where}: column {c + 1} has an empty name")
                    if name in columns[:c]:
                        raise ValueError(f"{where}: the column name '{name}' is given twice")
                values = np.full((len(names), len(columns)), np.nan)
                continue
            if len(fields) != len(columns) + 1:
                raise ValueError(f"{where}: {len(fields)} fields, not {len(columns) + 1}")
            s = index.get(fields[0])
            if s is None:
                skipped += 1
                continue
            if s in seen:
                raise ValueError(f"{where}: the sample '{fields[0]}' is given twice (first on line {seen[s]})")
            seen[s] = number
            for c, text in enumerate(fields[1:]):
                if text in ("", "NA"):
                    continue
                if not _NUMBER.fullmatch(text):
                    raise ValueError(f"{where}, column {columns[c]}: '{text}' is not a number, empty or NA")
                value = float(text)
                if value in (float("inf"), float("-inf")):
                    raise ValueError(f"{where}, column {columns[c]}: '{text}' overflows a double")
                values[s, c] = value
    if columns is None:
        raise ValueError(f"{path} has no header line")
    for s, name in enumerate(names):
        if s not in seen:
            raise ValueError(f"{path} has no line for the sample '{name}'")
    return columns, values, skipped


CORRELATION_HEADER = "edge_num\tcolumn\tmass_pearson\tmass_spearman\timbalance_pearson\timbalance_spearman"
DISPERSION_HEADER = ("edge_num\tmass_mean\tmass_var\tmass_sd\tmass_cv\tmass_vmr\timbalance_mean\timbalance_var\t"
                     "imbalance_sd")


def _g17_or_na(v) -> str:
    v = float(v)
    return "NA" if v != v else "%.17g" % v


def _na_or_float(text: str) -> float:
    return float(np.uint64(capi.NA_BITS).view(np.float64)) if text == "NA" else float(text)


def _used_head(what: str, names, totals, more: str = "", distance="kr"):
    totals = [int(x) for x in totals]
    if len(totals) != len(names):
        raise ValueError("one total mass per sample")
    lines = [f"# epik_amd {what} v1  samples={len(names)} used={sum(t != 0 for t in totals)}{more}" + _distance_field(distance)]
    return lines + [f"# unused\t{name}" for name, t in zip(names, totals) if t == 0]


def totals_of(mass) -> np.ndarray:
    """T_s of the rule: the wrapping sum of mass[s][:], uint64 [S]."""
    return np.asarray(mass, dtype=np.uint64).sum(axis=1, dtype=np.uint64)


def format_correlation_tsv(names, totals, columns, records, used) -> str:
    """cohort_correlation_<list>.tsv: the first line, a `# unused` line per sample without mass (`totals`[s] = T_s is 0), a
    `# column` line per column with its number of samples, the column names, then, long format, for every branch and every
    column the four correlations of records `capi.CORRELATION` [M][N]; doubles as %.17g, NA as NA."""
    records = np.asarray(records)
    if records.dtype != capi.CORRELATION or records.ndim != 2 or records.shape[0] != len(columns) or len(used) != len(columns):
        raise ValueError("records must be capi.CORRELATION [num_columns][num_branches], with one count per column")
    lines = _used_head("correlation", names, totals, f" columns={len(columns)}")
    lines += [f"# column\t{c}\t{name}\t{int(used[c])}" for c, name in enumerate(columns)]
    lines.append(CORRELATION_HEADER)
    for b in range(records.shape[1]):
        for c, name in enumerate(columns):
            lines.append(f"{b}\t{name}" + "".join("\t" + _g17_or_na(records[f][c, b]) for f in capi.CORRELATION.names))
    return "\n".join(lines) + "\n"


def _read_used_head(fh, what: str, pattern: str, path: str):
    head = re.fullmatch(rf"# epik_amd {what} v1  samples=(\d+) used=(\d+){pattern}", fh.readline().rstrip("\n"))
    if not head:
        raise ValueError(f"{path}: not a cohort {what} file")
    info = {"samples": int(head.group(1)), "used": int(head.group(2)), "unused": []}
    if head.groupdict().get("strata"):
        info["strata"] = head.group("strata")
    line = fh.readline().rstrip("\n")
    while line.startswith("# unused\t"):
        info["unused"].append(line.split("\t", 1)[1])
        line = fh.readline().rstrip("\n")
    if len(info["unused"]) != info["samples"] - info["used"]:
        raise ValueError(f"{path}: the unused samples do not follow the first line's counts")
    return head, info, line


def read_correlation_tsv(path: str):
    """(columns, records `capi.CORRELATION` [M][N], used uint32 [M], info {"samples", "used", "unused": names})"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(fh, "correlation", r" columns=(\d+)", path)
        columns, used = [], []
        while line.startswith("# column\t"):
            _, c, name, count = line.split("\t")
            if int(c) != len(columns):
                raise ValueError(f"{path}: the columns are not numbered in order")
            columns.append(name), used.append(int(count))
            line = fh.readline().rstrip("\n")
        if line != CORRELATION_HEADER or len(columns) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort correlation file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    m = len(columns)
    if len(rows) % m or any(len(r) != 6 for r in rows):
        raise ValueError(f"{path}: the rows do not follow the first line's counts")
    records = np.zeros((m, len(rows) // m), dtype=capi.CORRELATION)
    for i, r in enumerate(rows):
        if int(r[0]) != i // m or r[1] != columns[i % m]:
            raise ValueError(f"{path}: row {i} is out of order")
        records[i % m, i // m] = tuple(_na_or_float(x) for x in r[2:])
    return columns, records, np.array(used, dtype=np.uint32), info


def format_dispersion_tsv(names, totals, records) -> str:
    """cohort_dispersion_<list>.tsv: the first line, the `# unused` lines, the column names, then per branch the eight
    fields of records `capi.DISPERSION` [N]; doubles as %.17g, NA as NA."""
    records = np.asarray(records)
    if records.dtype != capi.DISPERSION or records.ndim != 1:
        raise ValueError("records must be capi.DISPERSION [num_branches]")
    lines = _used_head("dispersion", names, totals)
    lines.append(DISPERSION_HEADER)
    for b in range(records.shape[0]):
        lines.append(str(b) + "".join("\t" + _g17_or_na(records[f][b]) for f in capi.DISPERSION.names))
    return "\n".join(lines) + "\n"


def read_dispersion_tsv(path: str):
    """(records `capi.DISPERSION` [N], info {"samples", "used", "unused": names})"""
    with open(path, newline="") as fh:
        _, info, line = _read_used_head(fh, "dispersion", "", path)
        if line != DISPERSION_HEADER:
            raise ValueError(f"{path}: not a cohort dispersion file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if any(len(r) != 9 or int(r[0]) != i for i, r in enumerate(rows)):
        raise ValueError(f"{path}: the rows are not one per branch in order")
    records = np.zeros(len(rows), dtype=capi.DISPERSION)
    for i, r in enumerate(rows):
        records[i] = tuple(_na_or_float(x) for x in r[1:])
    return records, info


def read_factors(path: str, names, pairwise: bool = False, most: int | None = None):
    """The factor file of --cohort-permanova for the samples `names` of the list: (columns, uint32 labels [S][M] in list
    order with 0xffffffff for a missing one, label_names [M][id], the number of lines skipped because their sample is not in
    the list).  A TSV as `read_metadata`'s, but a value is a label: any non-empty text without a tab; empty or `NA` is
    missing.  A column's labels are numbered by first appearance in the file among the list's samples.  ValueError naming the
    line, and the column where there is one, for a wrong field count, a sample given twice or a column with more than 256
    distinct labels (32 with `pairwise`; `most`, where given, is the cap instead: 32 for --cohort-edge-test), and naming the
    sample of the list that the file lacks."""
    index = {name: s for s, name in enumerate(names)}
    capped = most is not None
    if not capped:
        most = capi.PERMANOVA_MAX_PAIR_GROUPS if pairwise else capi.PERMANOVA_MAX_GROUPS
    columns, labels, label_names, ids, seen, skipped = None, None, None, None, {}, 0
    with open(path, newline="") as fh:
        for number, line in enumerate(fh, 1):
            line = line.rstrip("\n")
            if line.endswith("\r"):
                line = line[:-1]
            if not line or line.startswith("#"):
                continue
            where = f"{path} line {number}"
            fields = line.split("\t")
            if columns is None:
                if fields[0] != "sample":
                    raise ValueError(f"{where}: the header must begin with 'sample'")
                if not 2 <= len(fields) <= 1 + capi.PERMANOVA_MAX_COLUMNS:
                    raise ValueError(f"{where}: the header names {len(fields) - 1} columns, not 1 to 64")
                columns = fields[1:]
                for c, name in enumerate(columns):
                    if not name:
                        raise ValueError(f"{where}: column {c + 1} has an empty name")
                    if name in columns[:c]:
                        raise ValueError(f"{where}: the column name '{name}' is given twice")
                labels = np.full((len(names), len(columns)), capi.PERMANOVA_MISSING, dtype=np.uint32)
                label_names, ids = [[] for _ in columns], [{} for _ in columns]
                continue
            if len(fields) != len(columns) + 1:
                raise ValueError(f"{where}: {len(fields)} fields, not {len(columns) + 1}")
            s = index.get(fields[0])
            if s is None:
                skipped += 1
                continue
            if s in seen:
                raise ValueError(f"{where}: the sample '{fields[0]}' is given twice (first on line {seen[s]})")
            seen[s] = number
            for c, text in enumerate(fields[1:]):
                if text in ("", "NA"):
                    continue
                if text not in ids[c]:
                    if len(label_names[c]) == most:
                        raise ValueError(f"{where}, column {columns[c]}: '{text}' is label number {most + 1}, more than {most}" +
                                         (" (the most of --cohort-permanova-pairwise)" if pairwise and not capped else ""))
                    ids[c][text] = len(label_names[c])
                    label_names[c].append(text)
                labels[s, c] = ids[c][text]
    if columns is None:
        raise ValueError(f"{path} has no header line")
    for s, name in enumerate(names):
        if s not in seen:
            raise ValueError(f"{path} has no line for the sample '{name}'")
    return columns, labels, label_names, skipped


def read_strata(path: str, names, column: str | None = None):
    """The strata of --cohort-strata FILE [--cohort-strata-column NAME] for the samples `names` of the list: (uint32 strata [S],
    the column's name).  FILE is read by `read_factors` (its errors) without a cap on the labels; `column` may be None only if
    FILE has one column.  ValueError too for a column that FILE lacks and, naming the line, for a sample without a value."""
    columns, labels, _, _ = read_factors(path, names, most=1 << 32)
    if column is None:
        if len(columns) != 1:
            raise ValueError(f"{path} has {len(columns)} columns: --cohort-strata-column must name one")
        c = 0
    elif column in columns:
        c = columns.index(column)
    else:
        raise ValueError(f"--cohort-strata-column: {path} has no column '{column}'")
    for s in np.flatnonzero(labels[:, c] == capi.PERMANOVA_MISSING):
        with open(path, newline="") as fh:
            number = next(n for n, line in enumerate(fh, 1) if line[:1] != "#" and line.rstrip("\r\n").split("\t")[0] == names[s])
        raise ValueError(f"{path} line {number}, column {columns[c]}: the sample '{names[s]}' has no stratum")
    return np.ascontiguousarray(labels[:, c]), columns[c]


def with_strata_field(text: str, strata) -> str:
    """A cohort_permanova, _permdisp, _edgetest or _model file's text with <TAB>strata=NAME at the end of its first line (after
    distance=.. where that is there): what --cohort-strata makes of the four files.  None or "" leaves the text as it is."""
    if not strata:
        return text
    at = text.find("\n")
    at = len(text) if at < 0 else at
    return text[:at] + f"\tstrata={strata}" + text[at:]


def constant_within_strata(column_labels, totals, strata, missing=0xFFFFFFFF) -> bool:
    """Whether a column's labels are constant inside every stratum among the samples with mass and a label: nothing can be
    permuted there, and the drivers warn."""
    seen = {}
    for v, t, h in zip(column_labels, totals, strata):
        if int(t) == 0 or int(v) == missing:
            continue
        if seen.setdefault(int(h), int(v)) != int(v):
            return False
    return True


PERMANOVA_HEADER = "column\ta\tb\tused\tgroups\tss_total\tss_among\tss_within\tf\tr2\tat_most\tp"


def groups_of(labels, totals):
    """The groups of every column in the rule's order: [(label ids by group, sizes by group)] per column, the groups numbered
    by first appearance among the samples with mass and a label."""
    labels, out = np.asarray(labels), []
    for c in range(labels.shape[1]):
        order, sizes = [], {}
        for s in range(labels.shape[0]):
            v = int(labels[s, c])
            if int(totals[s]) == 0 or v == capi.PERMANOVA_MISSING:
                continue
            if v not in sizes:
                order.append(v)
                sizes[v] = 0
            sizes[v] += 1
        out.append((order, [sizes[v] for v in order]))
    return out


def format_permanova_tsv(names, totals, columns, label_names, labels, permutations: int, seed: int, pairwise: bool, records,
                         group_ss, distance="kr", strata=None) -> str:
    """cohort_permanova_<list>.tsv: the first line, a `# unused` line per sample without mass, a `# column` line per column
    (its used samples and groups), a `# group` line per group (label, size, W_g / n_g of the observed labelling), the column
    names, then per column the whole test (a = b = *) and, with pairwise, its pairs in slot order; ss_among is
    ss_total - ss_within; doubles as %.17g, NA as NA.  `strata`: the name of the column of --cohort-strata, <TAB>strata=NAME at the
    end of the first line."""
    records, labels = np.asarray(records), np.asarray(labels)
    slots = 1 + (capi.PERMANOVA_PAIR_SLOTS if pairwise else 0)
    if records.dtype != capi.PERMANOVA or records.shape != (len(columns), slots) or labels.shape != (len(names), len(columns)):
        raise ValueError("records must be capi.PERMANOVA [num_columns][1 + Q], labels [num_samples][num_columns]")
    lines = _used_head("permanova", names, totals,
                       f" columns={len(columns)} permutations={int(permutations)} seed={int(seed)} pairwise={int(bool(pairwise))}",
                       distance)
    groups = groups_of(labels, totals)
    lines += [f"# column\t{c}\t{name}\t{int(records['used'][c, 0])}\t{int(records['groups'][c, 0])}" for c, name in enumerate(columns)]
    for c, (order, sizes) in enumerate(groups):
        lines += [f"# group\t{c}\t{g}\t{label_names[c][v]}\t{sizes[g]}\t{_g17_or_na(group_ss[c][g])}" for g, v in enumerate(order)]
    lines.append(PERMANOVA_HEADER)

    def line(c, a, b, r):
        total, within = float(r["ss_total"]), float(r["ss_within"])
        among = total if total != total else total - within
        return "\t".join([columns[c], a, b, str(int(r["used"])), str(int(r["groups"])), _g17_or_na(total), _g17_or_na(among),
                          _g17_or_na(within), _g17_or_na(r["f"]), _g17_or_na(r["r2"]), str(int(r["at_most"])), _g17_or_na(r["p"])])

    for c, (order, _) in enumerate(groups):
        lines.append(line(c, "*", "*", records[c, 0]))
        if pairwise:
            for h in range(1, len(order)):
                for g in range(h):
                    lines.append(line(c, label_names[c][order[g]], label_names[c][order[h]], records[c, pair_slot(g, h)]))
    return with_strata_field("\n".join(lines) + "\n", strata)


PERMDISP_HEADER = "column\ta\tb\tused\tgroups\tclipped\teta2\tf\tat_least\tp"


def format_permdisp_tsv(names, totals, columns, label_names, labels, permutations: int, seed: int, pairwise: bool, records,
                        group_mean, z, distance="kr", strata=None) -> str:
    """cohort_permdisp_<list>.tsv: the first line, the `# unused`, `# column` and `# group` lines as cohort_permanova's (a
    group's last field is its mean distance to centroid), the column names, per column the whole test (a = b = *) and, with
    pairwise, its pairs in slot order; then `# distances`, the column names column name label distance and, per column, a
    line per sample with mass and a label, in list order; doubles as %.17g, NA as NA.  Over a `distance` other than KR the
    first line ends in <TAB>distance=NAME.  `strata`: the name of the column of --cohort-strata, <TAB>strata=NAME at the
    end of the first line."""
    records, labels = np.asarray(records), np.asarray(labels)
    slots = 1 + (capi.PERMDISP_PAIR_SLOTS if pairwise else 0)
    if records.dtype != capi.PERMDISP or records.shape != (len(columns), slots) or labels.shape != (len(names), len(columns)):
        raise ValueError("records must be capi.PERMDISP [num_columns][1 + Q], labels [num_samples][num_columns]")
    lines = _used_head("permdisp", names, totals,
                       f" columns={len(columns)} permutations={int(permutations)} seed={int(seed)} pairwise={int(bool(pairwise))}",
                       distance)
    groups = groups_of(labels, totals)
    lines += [f"# column\t{c}\t{name}\t{int(records['used'][c, 0])}\t{int(records['groups'][c, 0])}" for c, name in enumerate(columns)]
    for c, (order, sizes) in enumerate(groups):
        lines += [f"# group\t{c}\t{g}\t{label_names[c][v]}\t{sizes[g]}\t{_g17_or_na(group_mean[c][g])}" for g, v in enumerate(order)]
    lines.append(PERMDISP_HEADER)

    def line(c, a, b, r):
        return "\t".join([columns[c], a, b, str(int(r["used"])), str(int(r["groups"])), str(int(r["clipped"])), _g17_or_na(r["eta2"]),
                          _g17_or_na(r["f"]), str(int(r["at_least"])), _g17_or_na(r["p"])])

    for c, (order, _) in enumerate(groups):
        lines.append(line(c, "*", "*", records[c, 0]))
        if pairwise:
            for h in range(1, len(order)):
                for g in range(h):
                    lines.append(line(c, label_names[c][order[g]], label_names[c][order[h]], records[c, pair_slot(g, h)]))
    lines += ["# distances", "column\tname\tlabel\tdistance"]
    for c, column in enumerate(columns):
        for s, name in enumerate(names):
            v = int(labels[s, c])
            if int(totals[s]) != 0 and v != capi.PERMDISP_MISSING:
                lines.append(f"{column}\t{name}\t{label_names[c][v]}\t{_g17_or_na(z[c][s])}")
    return with_strata_field("\n".join(lines) + "\n", strata)


def read_permanova_tsv(path: str):
    """(columns, rows [(column, a, b, record `capi.PERMANOVA`, ss_among)], groups [(c, g, label, n, ss_within_g)],
    info {"samples", "used", "unused", "permutations", "seed", "pairwise", "column_used", "column_groups"; and "distance", a
    name of `DISTANCES`, only where the first line has the field: a file over KR has none})"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(fh, "permanova", r" columns=(\d+) permutations=(\d+) seed=(\d+) pairwise=([01])"
                                           + _DISTANCE_FIELD + _STRATA_FIELD, path)
        info.update(permutations=int(head.group(4)), seed=int(head.group(5)), pairwise=head.group(6) == "1", column_used=[],
                    column_groups=[])
        if head.group(7):                     # (a file over KR has no such field, and its info no such key)
            info["distance"] = head.group(7)
        columns, groups = [], []
        while line.startswith("# column\t"):
            _, c, name, used, count = line.split("\t")
            if int(c) != len(columns):
                raise ValueError(f"{path}: the columns are not numbered in order")
            columns.append(name), info["column_used"].append(int(used)), info["column_groups"].append(int(count))
            line = fh.readline().rstrip("\n")
        while line.startswith("# group\t"):
            _, c, g, label, n, ss = line.split("\t")
            groups.append((int(c), int(g), label, int(n), _na_or_float(ss)))
            line = fh.readline().rstrip("\n")
        if line != PERMANOVA_HEADER or len(columns) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort permanova file")
        rows = []
        for ln in fh:
            r = ln.rstrip("\n").split("\t")
            if len(r) != 12 or r[0] not in columns:
                raise ValueError(f"{path}: not a row of a cohort permanova file: {ln!r}")
            record = np.zeros((), dtype=capi.PERMANOVA)
            record["used"], record["groups"], record["at_most"] = int(r[3]), int(r[4]), int(r[10])
            for f, text in zip(("ss_total", "ss_within", "f", "r2", "p"), (r[5], r[7], r[8], r[9], r[11])):
                record[f] = _na_or_float(text)
            rows.append((r[0], r[1], r[2], record, _na_or_float(r[6])))
    return columns, rows, groups, info


def read_permdisp_tsv(path: str):
    """(columns, rows [(column, a, b, record `capi.PERMDISP`)], groups [(c, g, label, n, mean_distance)], distances [(column,
    name, label, distance)], info as `read_permanova_tsv`'s)"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(fh, "permdisp", r" columns=(\d+) permutations=(\d+) seed=(\d+) pairwise=([01])"
                                           + _DISTANCE_FIELD + _STRATA_FIELD, path)
        info.update(permutations=int(head.group(4)), seed=int(head.group(5)), pairwise=head.group(6) == "1", column_used=[],
                    column_groups=[])
        if head.group(7):                     # (a file over KR has no such field, and its info no such key)
            info["distance"] = head.group(7)
        columns, groups = [], []
        while line.startswith("# column\t"):
            _, c, name, used, count = line.split("\t")
            if int(c) != len(columns):
                raise ValueError(f"{path}: the columns are not numbered in order")
            columns.append(name), info["column_used"].append(int(used)), info["column_groups"].append(int(count))
            line = fh.readline().rstrip("\n")
        while line.startswith("# group\t"):
            _, c, g, label, n, mean = line.split("\t")
            groups.append((int(c), int(g), label, int(n), _na_or_float(mean)))
            line = fh.readline().rstrip("\n")
        if line != PERMDISP_HEADER or len(columns) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort permdisp file")
        rows, distances, tail = [], [], False
        for ln in fh:
            r = ln.rstrip("\n").split("\t")
            if r == ["# distances"]:
                tail = True
                if fh.readline().rstrip("\n") != "column\tname\tlabel\tdistance":
                    raise ValueError(f"{path}: not a cohort permdisp file")
            elif tail and len(r) == 4 and r[0] in columns:
                distances.append((r[0], r[1], r[2], _na_or_float(r[3])))
            elif not tail and len(r) == 10 and r[0] in columns:
                record = np.zeros((), dtype=capi.PERMDISP)
                record["used"], record["groups"], record["clipped"], record["at_least"] = int(r[3]), int(r[4]), int(r[5]), int(r[8])
                for f, text in zip(("eta2", "f", "p"), (r[6], r[7], r[9])):
                    record[f] = _na_or_float(text)
                rows.append((r[0], r[1], r[2], record))
            else:
                raise ValueError(f"{path}: not a row of a cohort permdisp file: {ln!r}")
    return columns, rows, groups, distances, info


EDGETEST_HEADER = "edge_num\tcolumn" + "".join(f"\t{kind}_{field}" for kind in ("mass", "imbalance")
                                               for field in ("eta2", "f", "p", "p_adj", "top", "h", "kw_p", "kw_p_adj"))


def format_edgetest_tsv(names, totals, columns, label_names, labels, permutations: int, seed: int, records, strata=None) -> str:
    """cohort_edgetest_<list>.tsv: the first line, a `# unused` line per sample without mass, a `# column` line per column
    (its used samples and groups), a `# group` line per group (label, size), the column names, then per column a line per
    branch with at least one defined family: eta2, F, p, p_adj, the label of the group with the largest mean, H and the
    Kruskal-Wallis p and p_adj, of the mass and then of the imbalance; doubles as %.17g, NA as NA.  `strata`: the name of the column of --cohort-strata, <TAB>strata=NAME at the
    end of the first line."""
    records, labels = np.asarray(records), np.asarray(labels)
    if records.dtype != capi.EDGETEST or records.ndim != 2 or records.shape[0] != len(columns) or \
            labels.shape != (len(names), len(columns)):
        raise ValueError("records must be capi.EDGETEST [num_columns][num_branches], labels [num_samples][num_columns]")
    lines = _used_head("edgetest", names, totals, f" columns={len(columns)} permutations={int(permutations)} seed={int(seed)}")
    groups = groups_of(labels, totals)
    lines += [f"# column\t{c}\t{name}\t{int(records['used'][c, 0])}\t{int(records['groups'][c, 0])}" for c, name in enumerate(columns)]
    for c, (order, sizes) in enumerate(groups):
        lines += [f"# group\t{c}\t{g}\t{label_names[c][v]}\t{sizes[g]}" for g, v in enumerate(order)]
    lines.append(EDGETEST_HEADER)
    for c, (order, _) in enumerate(groups):
        defined = ~np.isnan(records["family"]["eta2"][c]).all(axis=1)
        for b in np.flatnonzero(defined):
            r = records[c, b]
            fields = [str(int(b)), columns[c]]
            for kind, top in ((0, int(r["top_mass"])), (1, int(r["top_imbalance"]))):
                plain, ranks = r["family"][2 * kind], r["family"][2 * kind + 1]
                fields += [_g17_or_na(plain["eta2"]), _g17_or_na(plain["stat"]), _g17_or_na(plain["p"]), _g17_or_na(plain["p_adj"]),
                           "NA" if top == capi.EDGETEST_MISSING else label_names[c][order[top]], _g17_or_na(ranks["stat"]),
                           _g17_or_na(ranks["p"]), _g17_or_na(ranks["p_adj"])]
            lines.append("\t".join(fields))
    return with_strata_field("\n".join(lines) + "\n", strata)


def read_edgetest_tsv(path: str):
    """(columns, rows [{"edge_num", "column", "mass_eta2", ..., "imbalance_kw_p_adj"}] with floats (nan for NA) and the
    `top` fields as labels (None for NA), groups [(c, g, label, n)], info {"samples", "used", "unused", "permutations",
    "seed", "column_used", "column_groups"})"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(fh, "edgetest", r" columns=(\d+) permutations=(\d+) seed=(\d+)" + _STRATA_FIELD, path)
        info.update(permutations=int(head.group(4)), seed=int(head.group(5)), column_used=[], column_groups=[])
        columns, groups = [], []
        while line.startswith("# column\t"):
            _, c, name, used, count = line.split("\t")
            if int(c) != len(columns):
                raise ValueError(f"{path}: the columns are not numbered in order")
            columns.append(name), info["column_used"].append(int(used)), info["column_groups"].append(int(count))
            line = fh.readline().rstrip("\n")
        while line.startswith("# group\t"):
            _, c, g, label, n = line.split("\t")
            groups.append((int(c), int(g), label, int(n)))
            line = fh.readline().rstrip("\n")
        if line != EDGETEST_HEADER or len(columns) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort edgetest file")
        keys, rows = EDGETEST_HEADER.split("\t"), []
        for ln in fh:
            r = ln.rstrip("\n").split("\t")
            if len(r) != len(keys) or r[1] not in columns:
                raise ValueError(f"{path}: not a row of a cohort edgetest file: {ln!r}")
            row = {"edge_num": int(r[0]), "column": r[1]}
            for key, text in zip(keys[2:], r[2:]):
                row[key] = (None if text == "NA" else text) if key.endswith("_top") else _na_or_float(text)
            rows.append(row)
    return columns, rows, groups, info


def read_samples_tsv(path: str):
    """(names, {column: uint64 array})"""
    with open(path, newline="") as fh:
        if fh.readline().rstrip("\n") != SAMPLES_HEADER:
            raise ValueError(f"{path}: not a cohort samples file")
        rows = [line.rstrip("\n").split("\t") for line in fh]
    cols = SAMPLES_HEADER.split("\t")[1:]
    return [r[0] for r in rows], {c: np.array([int(r[i + 1]) for r in rows], dtype=np.uint64) for i, c in enumerate(cols)}


def read_profile_tsv(path: str, names, num_branches: int):
    """(mass, best), uint64 [S][N], from the long-format file."""
    index = {name: s for s, name in enumerate(names)}
    mass = np.zeros((len(names), num_branches), np.uint64)
    best = np.zeros_like(mass)
    with open(path, newline="") as fh:
        if fh.readline().rstrip("\n") != PROFILE_HEADER:
            raise ValueError(f"{path}: not a cohort profile file")
        for line in fh:
            name, edge, b, m = line.rstrip("\n").split("\t")
            mass[index[name], int(edge)] = int(m)
            best[index[name], int(edge)] = int(b)
    return mass, best


def read_kr_tsv(path: str):
    """(names, float64 [S][S])"""
    with open(path, newline="") as fh:
        names = fh.readline().rstrip("\n").split("\t")[1:]
        rows = [line.rstrip("\n").split("\t") for line in fh]
    if [r[0] for r in rows] != names:
        raise ValueError(f"{path}: the rows do not follow the first line's names")
    return names, np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(names), len(names))


def read_unifrac_tsv(path: str):
    """(names, float64 [S][S]) of a cohort_unifrac_<metric>_<list>.tsv"""
    return read_kr_tsv(path)


def read_design(path: str, terms: str, names):
    """The design of --cohort-model for the samples `names` of the list: `path` a TSV in the layout of the factor file, `terms`
    the comma-separated f:NAME / n:NAME of --cohort-model-terms in test order.  (term names [T], kind uint32 [T], labels uint32
    [S][T], values float64 [S][T], label_names [T] by id, the number of lines skipped because their sample is not in the
    list).  ValueError as `read_cohort_design` of host/cohort.cpp raises its errors, naming the line and the column."""
    columns, kind = [], []
    for term in terms.split(","):
        where = f"--cohort-model-terms: term {len(columns) + 1} ('{term}')"
        if len(term) < 3 or term[1] != ":" or term[0] not in "fn":
            raise ValueError(f"{where} is not f:NAME (a factor) or n:NAME (numeric)")
        if term[2:] in columns:
            raise ValueError(f"{where}: the column '{term[2:]}' is given twice")
        if len(columns) == capi.MODEL_MAX_TERMS:
            raise ValueError("--cohort-model-terms: more than 16 terms")
        columns.append(term[2:]), kind.append(int(term[0] == "n"))
    t_count = len(columns)
    index = {name: s for s, name in enumerate(names)}
    labels = np.full((len(names), t_count), capi.MODEL_MISSING, dtype=np.uint32)
    values = np.full((len(names), t_count), np.nan)
    label_names, ids, seen, skipped, field_of, width = [[] for _ in columns], [{} for _ in columns], {}, 0, None, 0
    with open(path, newline="") as fh:
        for number, line in enumerate(fh, 1):
            line = line.rstrip("\n")
            if line.endswith("\r"):
                line = line[:-1]
            if not line or line.startswith("#"):
                continue
            where = f"{path} line {number}"
            fields = line.split("\t")
            if field_of is None:
                if fields[0] != "sample":
                    raise ValueError(f"{where}: the header must begin with 'sample'")
                if len(fields) < 2:
                    raise ValueError(f"{where}: the header names no column")
                for c, name in enumerate(fields[1:]):
                    if not name:
                        raise ValueError(f"{where}: column {c + 1} has an empty name")
                    if name in fields[1:c + 1]:
                        raise ValueError(f"{where}: the column name '{name}' is given twice")
                for t, name in enumerate(columns):
                    if name not in fields[1:]:
                        raise ValueError(f"{where}: the header has no column '{name}' (term {t + 1} of --cohort-model-terms)")
                field_of, width = [fields.index(name, 1) for name in columns], len(fields)
                continue
            if len(fields) != width:
                raise ValueError(f"{where}: {len(fields)} fields, not {width}")
            s = index.get(fields[0])
            if s is None:
                skipped += 1
                continue
            if s in seen:
                raise ValueError(f"{where}: the sample '{fields[0]}' is given twice (first on line {seen[s]})")
            seen[s] = number
            for t in range(t_count):
                text = fields[field_of[t]]
                if text in ("", "NA"):
                    continue
                at = f"{where}, column {columns[t]}: "
                if kind[t]:
                    if not _NUMBER.fullmatch(text):
                        raise ValueError(f"{at}'{text}' is not a number, empty or NA")
                    value = float(text)
                    if value in (float("inf"), float("-inf")):
                        raise ValueError(f"{at}'{text}' overflows a double")
                    values[s, t] = value
                    continue
                if text not in ids[t]:
                    if len(label_names[t]) == capi.MODEL_MAX_GROUPS:
                        raise ValueError(f"{at}'{text}' is label number 33, more than 32")
                    ids[t][text] = len(label_names[t])
                    label_names[t].append(text)
                labels[s, t] = ids[t][text]
    if field_of is None:
        raise ValueError(f"{path} has no header line")
    for s, name in enumerate(names):
        if s not in seen:
            raise ValueError(f"{path} has no line for the sample '{name}'")
    return columns, np.array(kind, dtype=np.uint32), labels, values, label_names, skipped


MODEL_HEADER = "term\tdf\tss\tr2\tf\tat_least\tp"


def _design_lines(names, totals, terms, kind, label_names, labels, values, term_columns, term_df, aliased):
    """The lines that cohort_model and cohort_edgemodel .tsv share: `# unused`, `# incomplete`, `# term`, `# group`, `# aliased`."""
    t_count = len(terms)
    lines = [f"# unused\t{name}" for name, t in zip(names, totals) if t == 0]
    lacks = np.where(kind[None, :] != 0, np.isnan(values), labels == capi.MODEL_MISSING)
    used = []
    for s, name in enumerate(names):
        if totals[s] == 0:
            continue
        if lacks[s].any():
            lines.append(f"# incomplete\t{name}\t{terms[int(np.argmax(lacks[s]))]}")
        else:
            used.append(s)
    lines += [f"# term\t{t}\t{'n' if kind[t] else 'f'}\t{terms[t]}\t{int(term_columns[t])}\t{int(term_df[t])}"
              for t in range(t_count)]
    column_of, groups = [], []
    for t in range(t_count):
        if kind[t]:
            column_of.append((t, "-"))
            continue
        order, sizes = [], {}
        for s in used:
            v = int(labels[s, t])
            if v not in sizes:
                order.append(v)
            sizes[v] = sizes.get(v, 0) + 1
        groups += [f"# group\t{t}\t{g}\t{label_names[t][v]}\t{sizes[v]}" for g, v in enumerate(order)]
        column_of += [(t, label_names[t][v]) for v in order[1:]]
    lines += groups
    lines += [f"# aliased\t{t}\t{label}" for c, (t, label) in enumerate(column_of[:capi.MODEL_MAX_COLUMNS]) if aliased[c]]
    return lines


def format_model_tsv(names, totals, terms, kind, label_names, labels, values, permutations: int, seed: int, model: Model,
                     distance="kr", strata=None) -> str:
    """cohort_model_<list>.tsv: the first line (used = the complete cases with mass), a `# unused` line per sample without mass,
    a `# incomplete` line per sample with mass that lacks a value (with the first term it lacks), a `# term` line per term, a
    `# group` line per group of a factor term in the rule's order, a `# aliased` line per dropped column, the column names, a
    line per term, then `model`, `residual` (df_res, ss_res, 1 less every term's r2 in one chain) and `total`; doubles as
    %.17g, NA as NA.  `strata`: the name of the column of --cohort-strata, <TAB>strata=NAME at the
    end of the first line."""
    kind, labels, values = np.asarray(kind), np.asarray(labels), np.asarray(values, dtype=np.float64)
    totals = [int(x) for x in totals]
    t_count, info, records = len(terms), model.info, model.records
    if labels.shape != (len(names), t_count) or values.shape != labels.shape or len(records) != t_count + 1 or len(totals) != len(names):
        raise ValueError("labels and values must be [num_samples][num_terms], the records [num_terms + 1]")
    lines = [f"# epik_amd model v1  samples={len(names)} used={int(info['used'])} terms={t_count} columns={int(info['columns'])} "
             f"rank={int(info['rank'])} permutations={int(permutations)} seed={int(seed)}" + _distance_field(distance)]
    lines += _design_lines(names, totals, terms, kind, label_names, labels, values, records['columns'], records['df'], model.aliased)
    lines.append(MODEL_HEADER)
    rest = np.float64(1.0)
    for k in range(t_count + 1):
        r = records[k]
        undefined = bool(np.isnan(r["p"]))
        lines.append("\t".join([terms[k] if k < t_count else "model", str(int(r["df"])), _g17_or_na(r["ss"]), _g17_or_na(r["r2"]),
                                _g17_or_na(r["f"]), "NA" if undefined else str(int(r["at_least"])), _g17_or_na(r["p"])]))
        if k < t_count and int(r["df"]) and not np.isnan(r["r2"]):
            rest = rest - np.float64(r["r2"])
    total = float(info["ss_total"]) > 0.0
    lines.append(f"residual\t{int(info['df_res'])}\t{_g17_or_na(info['ss_res'])}\t{_g17_or_na(rest) if total else 'NA'}\tNA\tNA\tNA")
    lines.append(f"total\t{int(info['used']) - 1}\t{_g17_or_na(info['ss_total'])}\t{'1' if total else 'NA'}\tNA\tNA\tNA")
    return with_strata_field("\n".join(lines) + "\n", strata)


def read_model_tsv(path: str):
    """(terms [(name, 'f' | 'n', columns, df)], records `capi.MODEL_TERM` [T + 1] (the model's last), info: samples, used,
    columns, rank, permutations, seed, unused, incomplete [(name, term)], groups [(term, g, label, n)], aliased [(term, label)],
    residual (df, ss, r2), total (df, ss, r2) and, over another distance than KR, distance)."""
    with open(path, newline="") as fh:
        first = fh.readline().rstrip("\n")
        head = re.fullmatch(r"# epik_amd model v1  samples=(\d+) used=(\d+) terms=(\d+) columns=(\d+) rank=(\d+) permutations=(\d+) "
                            r"seed=(\d+)" + _DISTANCE_FIELD + _STRATA_FIELD, first)
        if not head:
            raise ValueError(f"{path}: not a cohort model file")
        info = dict(samples=int(head.group(1)), used=int(head.group(2)), columns=int(head.group(4)), rank=int(head.group(5)),
                    permutations=int(head.group(6)), seed=int(head.group(7)), unused=[], incomplete=[], groups=[], aliased=[])
        if head.group(8):
            info["distance"] = head.group(8)
        if head.group("strata"):
            info["strata"] = head.group("strata")
        terms, rows = [], []
        line = fh.readline().rstrip("\n")
        while line.startswith("# "):
            r = line.split("\t")
            if r[0] == "# unused" and len(r) == 2:
                info["unused"].append(r[1])
            elif r[0] == "# incomplete" and len(r) == 3:
                info["incomplete"].append((r[1], r[2]))
            elif r[0] == "# term" and len(r) == 6 and int(r[1]) == len(terms):
                terms.append((r[3], r[2], int(r[4]), int(r[5])))
            elif r[0] == "# group" and len(r) == 5:
                info["groups"].append((int(r[1]), int(r[2]), r[3], int(r[4])))
            elif r[0] == "# aliased" and len(r) == 3:
                info["aliased"].append((int(r[1]), r[2]))
            else:
                raise ValueError(f"{path}: not a line of a cohort model file: {line!r}")
            line = fh.readline().rstrip("\n")
        if line != MODEL_HEADER or len(terms) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort model file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    if len(rows) != len(terms) + 3 or any(len(r) != 7 for r in rows) or [r[0] for r in rows[-3:]] != ["model", "residual", "total"]:
        raise ValueError(f"{path}: not a cohort model file")
    records = np.zeros(len(terms) + 1, dtype=capi.MODEL_TERM)
    for k, r in enumerate(rows[:-2]):
        records["df"][k] = int(r[1])
        records["columns"][k] = terms[k][2] if k < len(terms) else info["columns"]
        records["at_least"][k] = 0 if r[5] == "NA" else int(r[5])
        for f, text in zip(("ss", "r2", "f", "p"), (r[2], r[3], r[4], r[6])):
            records[f][k] = _na_or_float(text)
    for name, r in (("residual", rows[-2]), ("total", rows[-1])):
        info[name] = (int(r[1]), _na_or_float(r[2]), _na_or_float(r[3]))
    return terms, records, info


EDGEMODEL_FIELDS = ("ss", "r2", "partial_r2", "f", "sign", "p", "p_adj")
EDGEMODEL_HEADER = "term\tedge_num\t" + "\t".join(f"{k}_{f}" for k in ("mass", "imbalance") for f in EDGEMODEL_FIELDS)


def format_edgemodel_tsv(names, totals, terms, kind, label_names, labels, values, permutations: int, seed: int, result: Edgemodel,
                         strata=None) -> str:
    """cohort_edgemodel_<list>.tsv: the first line, the `# unused`, `# incomplete`, `# term`, `# group` and `# aliased` lines of
    cohort_model_<list>.tsv, the column names, then per term a line per branch with a defined family: the term, the branch and,
    for mass and imbalance, ss r2 partial_r2 f sign p p_adj; doubles as %.17g, NA as NA.  `strata`: as format_model_tsv's."""
    kind, labels, values = np.asarray(kind), np.asarray(labels), np.asarray(values, dtype=np.float64)
    totals = [int(x) for x in totals]
    t_count, info, records = len(terms), result.info, result.records
    if labels.shape != (len(names), t_count) or values.shape != labels.shape or records.shape[0] != t_count or len(totals) != len(names):
        raise ValueError("labels and values must be [num_samples][num_terms], the records [num_terms][num_branches]")
    lines = [f"# epik_amd edgemodel v1  samples={len(names)} used={int(info['used'])} terms={t_count} columns={int(info['columns'])} "
             f"rank={int(info['rank'])} permutations={int(permutations)} seed={int(seed)}"]
    lines += _design_lines(names, totals, terms, kind, label_names, labels, values, info["term_columns"], info["df"], result.aliased)
    lines.append(EDGEMODEL_HEADER)
    for t in range(t_count):
        for b in range(records.shape[1]):
            fams = records["family"][t, b]
            if np.isnan(fams["ss"]).all():
                continue
            cells = [terms[t], str(b)]
            for fam in fams:
                cells += [_g17_or_na(fam["ss"]), _g17_or_na(fam["r2"]), _g17_or_na(fam["partial_r2"]), _g17_or_na(fam["f"]),
                          "NA" if np.isnan(fam["ss"]) else str(int(fam["sign"])), _g17_or_na(fam["p"]), _g17_or_na(fam["p_adj"])]
            lines.append("\t".join(cells))
    return with_strata_field("\n".join(lines) + "\n", strata)


def read_edgemodel_tsv(path: str, num_branches: int):
    """(terms [(name, 'f' | 'n', columns, df)], records `capi.EDGEMODEL` [T][N] with ss, r2, partial_r2, f, sign, p and p_adj (NA
    for a branch without a line; the counts are not in the file), info: samples, used, columns, rank, permutations, seed, unused,
    incomplete, groups, aliased and, with strata, strata)."""
    with open(path, newline="") as fh:
        first = fh.readline().rstrip("\n")
        head = re.fullmatch(r"# epik_amd edgemodel v1  samples=(\d+) used=(\d+) terms=(\d+) columns=(\d+) rank=(\d+) permutations=(\d+) "
                            r"seed=(\d+)" + _STRATA_FIELD, first)
        if not head:
            raise ValueError(f"{path}: not a cohort edgemodel file")
        info = dict(samples=int(head.group(1)), used=int(head.group(2)), columns=int(head.group(4)), rank=int(head.group(5)),
                    permutations=int(head.group(6)), seed=int(head.group(7)), unused=[], incomplete=[], groups=[], aliased=[])
        if head.group("strata"):
            info["strata"] = head.group("strata")
        terms = []
        line = fh.readline().rstrip("\n")
        while line.startswith("# "):
            r = line.split("\t")
            if r[0] == "# unused" and len(r) == 2:
                info["unused"].append(r[1])
            elif r[0] == "# incomplete" and len(r) == 3:
                info["incomplete"].append((r[1], r[2]))
            elif r[0] == "# term" and len(r) == 6 and int(r[1]) == len(terms):
                terms.append((r[3], r[2], int(r[4]), int(r[5])))
            elif r[0] == "# group" and len(r) == 5:
                info["groups"].append((int(r[1]), int(r[2]), r[3], int(r[4])))
            elif r[0] == "# aliased" and len(r) == 3:
                info["aliased"].append((int(r[1]), r[2]))
            else:
                raise ValueError(f"{path}: not a line of a cohort edgemodel file: {line!r}")
            line = fh.readline().rstrip("\n")
        if line != EDGEMODEL_HEADER or len(terms) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort edgemodel file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    records = np.zeros((len(terms), num_branches), dtype=capi.EDGEMODEL)
    for f in EDGEMODEL_FIELDS:
        if f != "sign":
            records["family"][f] = _na_or_float("NA")
    index = {name: t for t, (name, _, _, _) in enumerate(terms)}
    for r in rows:
        if len(r) != 16 or r[0] not in index or not 0 <= int(r[1]) < num_branches:
            raise ValueError(f"{path}: not a line of a cohort edgemodel file: {r!r}")
        for k in range(2):
            for f, text in zip(EDGEMODEL_FIELDS, r[2 + 7 * k:9 + 7 * k]):
                records["family"][f][index[r[0]], int(r[1]), k] = (0 if text == "NA" else int(text)) if f == "sign" else _na_or_float(text)
    return terms, records, info


MANTEL_HEADER = "side\tmethod\tused\tr\tr_xz\tr_yz\tstat\tat_least\tp"
ANOSIM_HEADER = "column\tused\tgroups\tmean_between\tmean_within\tr\tat_least\tp"
_METHOD_NAMES = {1: "pearson", 2: "spearman", 3: "both"}


def format_mantel_tsv(names, totals, side_names, num_columns: int, methods, control, permutations: int, seed: int, records,
                      distance="kr", strata=None) -> str:
    """cohort_mantel_<list>.tsv: the first line (sides, permutations, seed, method, partial=NAME or -), the `# unused` lines, a
    `# side` line per side (the first `num_columns` are columns, the others matrices) with the samples of its first test, the
    column names, then a line per test of records `capi.MANTEL` [tests]; doubles as %.17g, NA as NA.  `methods`: pearson,
    spearman, both or the bits; `control`: a side index or None."""
    bits = methods if isinstance(methods, int) else {v: k for k, v in _METHOD_NAMES.items()}[methods]
    per_side = bin(bits).count("1")
    records = np.asarray(records)
    if records.dtype != capi.MANTEL or records.shape != (len(side_names) * per_side,):
        raise ValueError("records must be capi.MANTEL [sides * methods]")
    more = (f" sides={len(side_names)} permutations={int(permutations)} seed={int(seed)} method={_METHOD_NAMES[bits]}"
            f" partial={'-' if control is None else side_names[control]}")
    lines = _used_head("mantel", names, totals, more, distance)
    lines += [f"# side\t{q}\t{'column' if q < num_columns else 'matrix'}\t{name}\t{int(records['used'][q * per_side])}"
              for q, name in enumerate(side_names)]
    lines.append(MANTEL_HEADER)
    for r in records:
        lines.append("\t".join([side_names[int(r["side"])], "spearman" if r["method"] else "pearson", str(int(r["used"])),
                                _g17_or_na(r["r"]), _g17_or_na(r["r_xz"]), _g17_or_na(r["r_yz"]), _g17_or_na(r["stat"]),
                                str(int(r["at_least"])), _g17_or_na(r["p"])]))
    return with_strata_field("\n".join(lines) + "\n", strata)


def format_anosim_tsv(names, totals, columns, label_names, labels, permutations: int, seed: int, records, distance="kr",
                      strata=None) -> str:
    """cohort_anosim_<list>.tsv: the first line, the `# unused`, `# column` and `# group` lines as cohort_permanova's (a group
    line ends in its size), the column names, then a line per column of records `capi.ANOSIM` [M]."""
    records = np.asarray(records)
    if records.dtype != capi.ANOSIM or records.shape != (len(columns),):
        raise ValueError("records must be capi.ANOSIM [num_columns]")
    lines = _used_head("anosim", names, totals, f" columns={len(columns)} permutations={int(permutations)} seed={int(seed)}", distance)
    lines += [f"# column\t{c}\t{name}\t{int(records['used'][c])}\t{int(records['groups'][c])}" for c, name in enumerate(columns)]
    for c, (order, sizes) in enumerate(groups_of(labels, totals)):
        lines += [f"# group\t{c}\t{g}\t{label_names[c][v]}\t{n}" for g, (v, n) in enumerate(zip(order, sizes))]
    lines.append(ANOSIM_HEADER)
    for name, r in zip(columns, records):
        lines.append("\t".join([name, str(int(r["used"])), str(int(r["groups"])), _g17_or_na(r["mean_between"]),
                                _g17_or_na(r["mean_within"]), _g17_or_na(r["r"]), str(int(r["at_least"])), _g17_or_na(r["p"])]))
    return with_strata_field("\n".join(lines) + "\n", strata)


_TAIL = r"(?:\tdistance=(?P<distance>\w+))?(?:\tstrata=(?P<strata>[^\t]+))?"


def read_mantel_tsv(path: str):
    """(side names, kinds "column" | "matrix", records `capi.MANTEL` [tests], info {"samples", "used", "unused", "permutations",
    "seed", "method", "partial", "distance", "strata"})"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(
            fh, "mantel", r" sides=(\d+) permutations=(\d+) seed=(\d+) method=(pearson|spearman|both) partial=([^\t]+)" + _TAIL, path)
        sides, kinds = [], []
        while line.startswith("# side\t"):
            _, q, kind, name, _used = line.split("\t")
            if int(q) != len(sides) or kind not in ("column", "matrix"):
                raise ValueError(f"{path}: the sides are not numbered in order")
            sides.append(name), kinds.append(kind)
            line = fh.readline().rstrip("\n")
        if line != MANTEL_HEADER or len(sides) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort mantel file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    info.update(permutations=int(head.group(4)), seed=int(head.group(5)), method=head.group(6),
                partial=None if head.group(7) == "-" else head.group(7), distance=head.group("distance") or "kr")
    records = np.zeros(len(rows), dtype=capi.MANTEL)
    for i, r in enumerate(rows):
        if len(r) != 9 or r[0] not in sides or r[1] not in ("pearson", "spearman"):
            raise ValueError(f"{path}: row {i} is no test")
        side = sides.index(r[0])
        records[i] = (int(r[2]), side, r[1] == "spearman", info["partial"] is not None and r[0] != info["partial"], int(r[7]),
                      *(_na_or_float(x) for x in r[3:7]), _na_or_float(r[8]))
    return sides, kinds, records, info


def read_anosim_tsv(path: str):
    """(columns, groups [(label, n)] per column, records `capi.ANOSIM` [M], info)"""
    with open(path, newline="") as fh:
        head, info, line = _read_used_head(fh, "anosim", r" columns=(\d+) permutations=(\d+) seed=(\d+)" + _TAIL, path)
        columns, groups = [], []
        while line.startswith("# column\t"):
            columns.append(line.split("\t")[2]), groups.append([])
            line = fh.readline().rstrip("\n")
        while line.startswith("# group\t"):
            _, c, g, label, n = line.split("\t")
            if int(g) != len(groups[int(c)]):
                raise ValueError(f"{path}: the groups are not numbered in order")
            groups[int(c)].append((label, int(n)))
            line = fh.readline().rstrip("\n")
        if line != ANOSIM_HEADER or len(columns) != int(head.group(3)):
            raise ValueError(f"{path}: not a cohort anosim file")
        rows = [ln.rstrip("\n").split("\t") for ln in fh]
    info.update(permutations=int(head.group(4)), seed=int(head.group(5)), distance=head.group("distance") or "kr")
    if [r[0] for r in rows] != columns or any(len(r) != 8 for r in rows):
        raise ValueError(f"{path}: the rows do not follow the columns")
    records = np.zeros(len(rows), dtype=capi.ANOSIM)
    for i, r in enumerate(rows):
        records[i] = (int(r[1]), int(r[2]), int(r[6]), _na_or_float(r[5]), _na_or_float(r[3]), _na_or_float(r[4]), _na_or_float(r[7]))
    return columns, groups, records, info
