"""Edge principal components of a cohort's samples, no device: the rule of include/epik_amd.h restated here in numpy, a
round's rotations vectorised, against epik_amd_cohort_epca_host -- every byte of mu, proj, edge and the info block --, a
case derived by hand, forged cohorts, properties on random cohorts (numpy.linalg.eigh among them), the C ABI's refusals,
the drivers' and the launcher's flags, the two files and the stand-alone host binary (plain and under ASan + UBSan).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, random_cells, same_bits, tree_case  # noqa: F401 (host_bins: a fixture)
from test_squash_cpu import BALANCED, numpy_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
EPS = 2.0 ** -52
MAX_SWEEPS = 64


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def sequential_sum(terms, axis):
    """acc = +0.0, then acc = acc + term along `axis` in ascending order: np.add.accumulate adds one element after the
    other, and starts from its first term where the rule starts from +0.0 -- the two differ when that term is -0.0 --, so
    a +0.0 goes in front."""
    shape = list(terms.shape)
    shape[axis] = 1
    return np.take(np.add.accumulate(np.concatenate([np.zeros(shape), terms], axis=axis), axis=axis), -1, axis=axis)


def numpy_gram(mass, first):
    """(used, Y [L][N], G [L][L], scale, trace) of the rule."""
    mass = np.asarray(mass, dtype=U64)
    n = mass.shape[1]
    first = np.asarray(first, dtype=np.int64)
    c, b, total = numpy_planes(mass, first)
    used = np.flatnonzero(total > 0)
    count = len(used)
    inner = first < np.arange(n)
    x = np.where(inner[None, :], (b[used] + c[used]) - 1.0, 0.0)
    if count:
        y = x - (sequential_sum(x, 0) / np.float64(count))[None, :]
    else:
        y = x
    g = np.zeros((count, count))
    for i in range(count):          # G[i][j]: the sum over b in order; a product commutes bit for bit, so does the mirror
        g[i] = sequential_sum(y[i][None, :] * y, 1)
    scale = np.float64(g.diagonal().max()) if count else np.float64(0.0)
    return used, y, g, scale, np.float64(sequential_sum(g.diagonal().copy(), 0))


def round_pairs(m, r):
    """The pairs (p, q), p < q, of round r over m indices (m even)."""
    i = np.arange(1, m // 2)
    x = np.concatenate([[r], (r + i) % (m - 1)])
    y = np.concatenate([[m - 1], (r - i + m - 1) % (m - 1)])
    return np.minimum(x, y), np.maximum(x, y)


def numpy_jacobi(g, scale):
    """(A, V, sweeps, converged): cyclic Jacobi by the rule, the rotations of a round applied together."""
    count = len(g)
    a, v = g.copy(), np.eye(count)
    tol = EPS * scale
    m = count + count % 2
    upper = np.arange(count)[:, None] <= np.arange(count)[None, :]
    sweeps, converged = 0, 0
    while sweeps < MAX_SWEEPS and not converged:
        sweeps += 1
        rotated = 0
        for r in range(m - 1):
            p, q = round_pairs(m, r)
            real = q < count
            p, q = p[real], q[real]
            apq = a[p, q]
            turn = np.abs(apq) > tol
            p, q, apq = p[turn], q[turn], apq[turn]
            if not len(p):
                continue
            rotated += len(p)
            theta = (a[q, q] - a[p, p]) / (2.0 * apq)
            t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
            t = np.where(theta < 0, -t, t)
            c = 1.0 / np.sqrt(t * t + 1.0)
            s = t * c
            j, partner = np.concatenate([p, q]), np.concatenate([q, p])      # index p: (c, s, q); index q: (c, -s, p)
            cj, sj = np.concatenate([c, c]), np.concatenate([s, -s])
            a1, v1 = a.copy(), v.copy()
            a1[:, j] = cj[None, :] * a[:, j] - sj[None, :] * a[:, partner]  # the column phase, on the full matrix
            v1[:, j] = cj[None, :] * v[:, j] - sj[None, :] * v[:, partner]
            a2 = a1.copy()
            a2[j, :] = cj[:, None] * a1[j, :] - sj[:, None] * a1[partner, :]  # the row phase ...
            a2 = np.where(upper, a2, a2.T)                                    # ... holds for i <= j; the rest is its mirror
            a2[p, q] = a2[q, p] = 0.0
            a, v = a2, v1
        converged = int(rotated == 0)
    return a, v, sweeps, converged


def numpy_epca(mass, first, num_components):
    """(mu [K], proj [S][K], edge [K][N], info) by the header's text."""
    mass = np.asarray(mass, dtype=U64)
    s, n = mass.shape
    k_all = int(num_components)
    used, y, g, scale, trace = numpy_gram(mass, first)
    count = len(used)
    a, v, sweeps, converged = numpy_jacobi(g, scale)
    mu_all = a.diagonal().copy()
    order = np.lexsort((np.arange(count), -mu_all))                           # (mu descending, j ascending)
    kc = min(k_all, count)
    mu, proj, edge = np.zeros(k_all), np.zeros((s, k_all)), np.zeros((k_all, n))
    for k in range(kc):
        jk = order[k]
        mu[k] = mu_all[jk]
        if not mu[k] > 2.0 ** -40 * scale:
            continue
        r = np.sqrt(mu[k])
        raw = sequential_sum(v[:, jk][:, None] * y, 0)
        sign = -1.0 if raw[np.argmax(np.abs(raw))] < 0 else 1.0               # (argmax: the first of the largest)
        edge[k] = sign * (raw / r)
        proj[used, k] = sign * (v[:, jk] * r)
    info = np.zeros(1, dtype=capi.EPCA_INFO)
    info[0] = (count, kc, sweeps, converged, trace, scale)
    return mu, proj, edge, info[0]


def host_epca_raw(mass, first, k):
    """(mu, proj, edge, info) straight from the C entry, into poisoned buffers."""
    lib = capi.load()
    mass = np.ascontiguousarray(mass, dtype=U64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    s, n = mass.shape
    mu, proj, edge = np.zeros(k), np.zeros((s, k)), np.zeros((k, n))
    info = np.zeros(1, dtype=capi.EPCA_INFO)
    for buf in (mu, proj, edge, info):
        buf.view(np.uint8)[:] = 0xA5
    assert lib.epik_amd_cohort_epca_host(mass.ctypes.data, s, n, first.ctypes.data, k, mu.ctypes.data, proj.ctypes.data,
                                         edge.ctypes.data, info.ctypes.data) == capi.OK, lib.epik_amd_last_error()
    return mu, proj, edge, info[0]


def assert_epca(got, want, what=""):
    """Every byte of mu, proj, edge and the info block; `got` and `want` are tuples or `cohort.Epca`."""
    parts = []
    for x in (got, want):
        parts.append((x.mu, x.proj, x.edge, x.info) if isinstance(x, cohort_mod.Epca) else x)
    (mu, proj, edge, info), (w_mu, w_proj, w_edge, w_info) = parts
    assert np.asarray(info).tobytes() == np.asarray(w_info).tobytes(), (what, info, w_info)
    assert same_bits(mu, w_mu), (what, mu, w_mu)
    assert same_bits(proj, w_proj), (what, np.argwhere(np.asarray(proj).view(U64) != np.asarray(w_proj).view(U64))[:5])
    assert same_bits(edge, w_edge), (what, np.argwhere(np.asarray(edge).view(U64) != np.asarray(w_edge).view(U64))[:5])


RESTATED = {}


def restated(tree_name, num_samples):
    """(mass, first, {K: numpy_epca}) of a case of the first test, computed once."""
    key = (tree_name, num_samples)
    if key not in RESTATED:
        parent, _ = tree_case(tree_name)
        first = numpy_first(parent)
        mass = random_cells(np.random.default_rng(3000 + num_samples), num_samples, len(parent), empty=1, bits=42)
        RESTATED[key] = (mass, first, {k: numpy_epca(mass, first, k) for k in (1, 5, 64)})
    return RESTATED[key]


SAMPLES_AND_USED = {1: 1, 2: 1, 3: 2, 4: 3, 33: 32, 34: 33, 70: 69}


@pytest.mark.parametrize("tree_name", ["one", "tree15", "tree2999"])
@pytest.mark.parametrize("num_samples", sorted(SAMPLES_AND_USED))
def test_epca_host_equals_the_numpy_restatement_bit_for_bit(tree_name, num_samples):
    mass, first, wants = restated(tree_name, num_samples)
    for k, want in wants.items():
        got = host_epca_raw(mass, first, k)
        used = int((mass.sum(axis=1, dtype=U64) > 0).sum())
        assert int(got[3]["used"]) == used and int(got[3]["components"]) == min(k, used)
        # (one cell a sample on the tree of one branch: random_cells leaves more than one sample empty there)
        assert used == SAMPLES_AND_USED[num_samples] or tree_name == "one"
        assert_epca(got, want, (tree_name, num_samples, k))
        assert int(got[3]["converged"]) == 1 and int(got[3]["sweeps"]) <= MAX_SWEEPS
    assert_epca(cohort_mod.epca_host(mass, first, 5), wants[5])


# ---- a case by hand --------------------------------------------------------------------------------------------------
def test_two_samples_on_two_leaves_by_hand():
    # ((0,1)2,(3,4)5)6: A all on leaf 0, B all on leaf 3.  Inner branches 2, 5, 6.  X_A = (1, -1, 1), X_B = (-1, 1, 1):
    # the root has everything distal of it for both; mean = (0, 0, 1), Y = +-(1, -1, 0), G = [[2, -2], [-2, 2]].
    first = numpy_first(BALANCED)
    mass = np.zeros((2, 7), U64)
    mass[0, 0], mass[1, 3] = 9, 4
    used, y, g, scale, trace = numpy_gram(mass, first)
    assert same_bits(y[:, [2, 5, 6]], [[1, -1, 0], [-1, 1, 0]]) and not y[:, [0, 1, 3, 4]].any()
    assert same_bits(g, [[2, -2], [-2, 2]]) and scale == 2 and trace == 4
    got = cohort_mod.epca_host(mass, first, 2)
    assert_epca(got, numpy_epca(mass, first, 2))
    assert (int(got.info["used"]), int(got.info["components"]), int(got.info["converged"])) == (2, 2, 1)
    assert list(got.null()) == [False, True]
    # one component: mu = 4, the unit vector along (1, -1, 0), branch 2 positive by the sign rule, and the samples at
    # +-sqrt(2) on it.  The only inexact steps are 1 / sqrt(2) and its products: 4 ulp.
    root = np.sqrt(0.5)
    assert abs(got.mu[0] - 4.0) <= 4 * np.spacing(4.0)
    assert np.abs(got.edge[0, [2, 5, 6]] - [root, -root, 0.0]).max() <= 4 * np.spacing(root)       # (4 ulp of 1 / sqrt(2))
    assert not got.edge[0, [0, 1, 3, 4]].any()
    assert np.abs(got.proj[:, 0] - [np.sqrt(2.0), -np.sqrt(2.0)]).max() <= 4 * np.spacing(np.sqrt(2.0))  # (... of sqrt(2))
    assert not got.edge[1].view(U64).any() and not got.proj[:, 1].view(U64).any()


# ---- forged cohorts --------------------------------------------------------------------------------------------------
def forged_epca_cohorts():
    """name -> (mass, parent, K)"""
    parent, _ = tree_case("tree15")
    n = len(parent)
    rng = np.random.default_rng(43)
    x, y, z = (random_cells(rng, 1, n, bits=42)[0] for _ in range(3))
    zero = np.zeros(n, U64)
    leaf = np.zeros(n, U64)
    leaf[0] = 7
    star = np.array([3, 3, 3, -1])
    return {
        "all empty": (np.stack([zero, zero, zero]), parent, 5),
        # x + x is exact and so is its half: Y = 0 exactly
        "all identical": (np.stack([x, x]), parent, 5),
        # every X is 1, -1 or 0: the sums and the mean are exact whatever the count
        "four identical on a leaf": (np.stack([leaf, leaf * U64(3), leaf, leaf]), parent, 5),
        "two identical pairs": (np.stack([x, x, y, y]), parent, 5),
        "pairs and one more": (np.stack([x, y, x, z, y]), parent, 64),
        "no inner branch": (random_cells(rng, 3, 1, bits=42) + U64(1), tree_case("one")[0], 5),
        # the root is the only inner branch and carries no mass: X = 1 for every sample, 1 + 1 + 1 = 3 and 3 / 3 = 1 are exact
        "a star": ((random_cells(rng, 3, 4, bits=42) + U64(1)) * np.array([1, 1, 1, 0], U64), star, 5),
    }


@pytest.mark.parametrize("name", sorted(forged_epca_cohorts()))
def test_forged_cohorts(name):
    mass, parent, k = forged_epca_cohorts()[name]
    first = numpy_first(parent)
    want = numpy_epca(mass, first, k)
    got = host_epca_raw(mass, first, k)
    assert_epca(got, want, name)
    mu, proj, edge, info = got
    epca = cohort_mod.epca_host(mass, first, k)
    assert int(info["converged"]) == 1 and int(info["sweeps"]) <= MAX_SWEEPS
    nothing = lambda: not (mu.view(U64).any() or proj.view(U64).any() or edge.view(U64).any())
    if name == "all empty":
        assert tuple(info.tolist()) == (0, 0, 1, 1, 0.0, 0.0) and nothing()
    elif name in ("all identical", "four identical on a leaf", "no inner branch", "a star"):
        assert int(info["used"]) == len(mass) and int(info["sweeps"]) == 1 and epca.null().all()
        assert same_bits([info["trace"], info["scale"]], [0.0, 0.0]) and nothing()
    elif name == "two identical pairs":       # Y = +-(x - y) / 2 but for rounding: one real component, three near zero
        assert int(info["components"]) == 4 and list(epca.null()) == [False, True, True, True]
        assert not edge[1:].view(U64).any() and not proj[:, 1:].view(U64).any()
        assert np.abs(proj[0, 0] - proj[1, 0]) <= 1e-12 * abs(proj[0, 0]) and proj[0, 0] * proj[2, 0] < 0
    elif name == "pairs and one more":        # three distinct points: two real components
        assert int(info["components"]) == 5 and list(epca.null()) == [False, False, True, True, True]


# ---- properties on random cohorts ------------------------------------------------------------------------------------
# The largest |mu - w| / (2^-52 * L * mu_max) of the restatement against numpy.linalg.eigh of its own G over property_cases(),
# measured on the machine the test was written on: EIGH_MEASURED.  Both solvers are backward stable and the gap scales
# with L * eps * mu_max; the factor 8 covers another BLAS behind numpy.
EIGH_MEASURED = 1.12  # (0.709, 1.118, 1.118 and 0.760 over the four cases: eigh_gap())
EIGH_BOUND = 8 * EIGH_MEASURED


def property_cases():
    tree = synth.make_tree(40, seed=7)
    first = numpy_first(tree.parent)
    rng = np.random.default_rng(6)
    cases = [(random_cells(rng, s, len(first), empty=e, bits=50), first) for s, e in ((12, None), (33, 5), (20, 0))]
    mass, first, _ = restated("tree2999", 70)
    return cases + [(mass, first)]


def eigh_gap(mass, first):
    """|mu - w| / (2^-52 * L * mu_max), the largest over the spectrum, of the restatement's Jacobi against eigh."""
    _, _, g, scale, _ = numpy_gram(mass, first)
    a, _, _, _ = numpy_jacobi(g, scale)
    mu = np.sort(a.diagonal())
    w = np.linalg.eigh(g)[0]
    return np.abs(mu - w).max() / (EPS * len(g) * np.abs(w).max())


def test_properties_on_random_cohorts():
    for mass, first in property_cases():
        n = len(first)
        want = numpy_epca(mass, first, 64)
        got = cohort_mod.epca_host(mass, first, 64)
        assert_epca(got, want)
        info = got.info
        count, kc, sweeps = int(info["used"]), int(info["components"]), int(info["sweeps"])
        assert int(info["converged"]) == 1 and sweeps == int(want[3]["sweeps"]) and sweeps <= MAX_SWEEPS
        used, y, g, scale, trace = numpy_gram(mass, first)
        live = ~got.null()
        assert live.any() and (np.diff(got.mu[:kc]) <= 0).all()
        e, mu = got.edge[:kc][live], got.mu[:kc][live]
        # G differs from the exact Gram matrix of Y by at most N * eps * scale an entry (N products of at most scale in
        # magnitude, summed in order); Jacobi leaves off-diagonals of at most eps * scale and, backward stable, perturbs by
        # L * eps * scale a sweep; e_k . e_l = v_k' (Y Y') v_l / sqrt(mu_k mu_l).  A factor 4 for the sums behind raw[].
        slack = 4 * (n + count * sweeps) * EPS * float(scale)
        assert (np.abs(e @ e.T - np.eye(len(e))) <= slack / np.sqrt(mu[:, None] * mu[None, :])).all()
        # ... and proj[s][k] = Y_s . edge[k] = (G v_k)_s / r = v_k[s] * r
        assert (np.abs(y @ e.T - got.proj[used][:, :kc][:, live]) <= slack / np.sqrt(mu)[None, :]).all()
        assert not got.proj[np.setdiff1d(np.arange(len(mass)), used)].view(U64).any()
        w = np.linalg.eigh(g)[0][::-1]
        gap = np.abs(got.mu[:kc] - w[:kc]).max() / (EPS * count * np.abs(w).max())
        print(f"L = {count}, N = {n}: sweeps {sweeps}, eigh gap {gap:.3f} of 2^-52 L mu_max")
        assert gap <= EIGH_BOUND, (gap, EIGH_BOUND)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_epca_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    for name in ("epik_amd_cohort_epca_device", "epik_amd_cohort_epca", "epik_amd_cohort_epca_host"):
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3 and capi.EPCA_INFO.itemsize == 32
    fields = ("used", "components", "sweeps", "converged", "trace", "scale")
    assert [capi.EPCA_INFO.fields[k][1] for k in fields] == [0, 4, 8, 12, 16, 24]
    err = lambda: lib.epik_amd_last_error().decode()
    info = np.zeros(1, dtype=capi.EPCA_INFO)
    assert lib.epik_amd_cohort_epca_device(None, None, 5, None, None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_epca(None, None, 5, None, None, None, info.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    first = cohort_mod.first_of([2, 2, -1])
    mass = np.ones((2, 3), U64)
    mu, proj, edge = np.zeros(64), np.zeros((2, 64)), np.zeros((64, 3))
    host = lib.epik_amd_cohort_epca_host
    args = lambda m=mass, s=2, n=3, f=first, k=2, a=mu, p=proj, e=edge, i=info: (
        m.ctypes.data if m is not None else None, s, n, f.ctypes.data if f is not None else None, k,
        *(x.ctypes.data if x is not None else None for x in (a, p, e, i)))
    assert host(*args()) == capi.OK and int(info[0]["used"]) == 2 and int(info[0]["components"]) == 2
    assert host(*args(k=64)) == capi.OK
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(k=bad)) == capi.ERR_INVALID and "num_components" in err() and "[1, 64]" in err()
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    assert host(*args(n=0)) == capi.ERR_INVALID
    for missing in ("m", "f", "a", "p", "e", "i"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    above = np.array([0, 2, 0], dtype=np.uint32)
    assert host(*args(f=above)) == capi.ERR_INVALID and "branch 1" in err() and "first" in err()
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.epca_host(mass, first, 0)
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.epca_host(mass, first, 65)
    with pytest.raises(ValueError):
        cohort_mod.epca_host(mass, first[:2], 5)


# ---- the drivers and the launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_epca_without_cohort_and_name_the_flag(host_bins, tmp_path, binary):
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(tmp_path)]
    for extra, flag, needs in ((["--cohort-epca"], "--cohort-epca", "--cohort "),
                               (["--cohort-epca", "--cohort-epca-components", "3"], "--cohort-epca", "--cohort "),
                               (["--cohort", "--cohort-epca-components", "3"], "--cohort-epca-components", "--cohort-epca "),
                               (["--cohort", "--cohort-epca", "--cohort-epca-components", "0"], "--cohort-epca-components", "[1, 64]"),
                               (["--cohort", "--cohort-epca", "--cohort-epca-components", "65"], "--cohort-epca-components", "[1, 64]"),
                               (["--cohort", "--cohort-epca", "--cohort-epca-components", "x"], "--cohort-epca-components", "[1, 64]")):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr.startswith("Error:") and flag in run.stderr and needs in run.stderr, (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(tmp_path.iterdir())
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-epca " in out.stdout and "--cohort-epca-components" in out.stdout
    assert "cohort_epca_<list>.tsv" in out.stdout and "cohort_epca_edges_<list>.tsv" in out.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-epca" not in " ".join(default)
    assert epik.driver_command(**kw, cohort_epca=False, cohort_epca_components=None) == default
    assert "--cohort-epca" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort=True, cohort_epca=True)[:-1] == default[:-1] + ["--cohort", "--cohort-epca"]
    assert epik.driver_command(**kw, cohort=True, cohort_epca=True, cohort_epca_components=3)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-epca", "--cohort-epca-components", "3"]
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort_epca=True)
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort=True, cohort_epca_components=3)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-epca" in out.stdout and "--cohort-epca-components" in out.stdout
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort-epca", me], capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort" in run.stderr, (run.stdout, run.stderr)


def test_the_two_files_read_back_and_keep_names(tmp_path):
    names = ["a", "skin 3", "it's", "none", "z.9_-"]
    parent, _ = tree_case("tree15")
    first = numpy_first(parent)
    mass = random_cells(np.random.default_rng(8), 5, len(parent), bits=42)
    mass[3] = 0
    used = mass.sum(axis=1, dtype=U64) > 0
    epca = cohort_mod.epca_host(mass, first, 3)
    text = cohort_mod.format_epca_tsv(names, used, epca)
    lines = text.split("\n")
    assert lines[0] == f"# epik_amd epca v1  samples=5 used=4 components=3 sweeps={int(epca.info['sweeps'])} converged=1"
    assert lines[1] == "# unused\tnone" and lines[2].startswith("# component\t1\t%.17g\t" % epca.mu[0]) and lines[2].endswith("\tok")
    assert lines[5] == "name\tpc1\tpc2\tpc3" and [ln.split("\t")[0] for ln in lines[6:10]] == ["a", "skin 3", "it's", "z.9_-"]
    assert len(lines) == 11 and lines[-1] == ""
    comp = lines[3].split("\t")
    assert comp[1] == "2" and comp[3] == "%.17g" % (epca.mu[1] / 3.0) and comp[4] == "%.17g" % (epca.mu[1] / float(epca.info["trace"]))
    path = tmp_path / "cohort_epca_x.tsv"
    path.write_bytes(text.encode())
    back_names, proj, info = cohort_mod.read_epca_tsv(str(path))
    assert back_names == ["a", "skin 3", "it's", "z.9_-"] and info["unused"] == ["none"]
    assert same_bits(proj, epca.proj[used][:, :3]) and same_bits(info["mu"], epca.mu)      # %.17g reads back to the same double
    assert (info["samples"], info["used"], info["components"], info["converged"]) == (5, 4, 3, 1) and not info["null"].any()
    assert same_bits(info["lambda"], epca.mu / 3.0) and same_bits(info["fraction"], epca.mu / float(epca.info["trace"]))
    edges_text = cohort_mod.format_epca_edges_tsv(first, epca)
    inner = np.flatnonzero(first < np.arange(len(first)))
    assert edges_text.split("\n")[0] == "edge_num\tpc1\tpc2\tpc3" and edges_text.count("\n") == 1 + len(inner)
    edges_path = tmp_path / "cohort_epca_edges_x.tsv"
    edges_path.write_bytes(edges_text.encode())
    edge_num, coeff = cohort_mod.read_epca_edges_tsv(str(edges_path))
    assert list(edge_num) == list(inner) and same_bits(coeff, epca.edge[:3, inner].T)
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_epca_tsv(str(path))
    edges_path.write_text("name\tpc1\n")
    with pytest.raises(ValueError):
        cohort_mod.read_epca_edges_tsv(str(edges_path))
    with pytest.raises(ValueError):
        cohort_mod.format_epca_tsv(names, np.ones(5, bool), epca)
    # nothing used: the first line, the unused samples, the column of names alone
    empty = cohort_mod.epca_host(np.zeros((2, len(first)), U64), first, 5)
    assert cohort_mod.format_epca_tsv(["x y", "q"], [False, False], empty) == (
        "# epik_amd epca v1  samples=2 used=0 components=0 sweeps=1 converged=1\n# unused\tx y\n# unused\tq\nname\n")
    assert cohort_mod.format_epca_edges_tsv(first, empty).split("\n")[:2] == ["edge_num", str(int(inner[0]))]


# ---- the host code stand-alone -----------------------------------------------------------------------------------------
def _epca_input(path, mass, first):
    with open(path, "wb") as fh:
        fh.write(np.array(mass.shape, dtype="<u8").tobytes() + np.ascontiguousarray(mass, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.zeros(mass.shape[1]).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_epca_is_the_library_s(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    parent, _ = tree_case("tree15")
    first = numpy_first(parent)
    for num_samples in (1, 3, 7):
        mass = random_cells(np.random.default_rng(9), num_samples, len(parent), empty=1, bits=42)
        _epca_input(tmp_path / "in.bin", mass, first)
        run = subprocess.run([binary, "epca", str(tmp_path / "out.bin"), str(tmp_path / "in.bin"), "5"], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_samples, run.stderr)
        mu, proj, edge, info = host_epca_raw(mass, first, 5)
        want = mu.tobytes() + proj.tobytes() + edge.tobytes() + np.asarray(info).tobytes()
        assert (tmp_path / "out.bin").read_bytes() == want, num_samples
    for bad in ("0", "65"):
        run = subprocess.run([binary, "epca", str(tmp_path / "o.bin"), str(tmp_path / "in.bin"), bad], capture_output=True, text=True)
        assert run.returncode == 1 and "num_components" in run.stderr
