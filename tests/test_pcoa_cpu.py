"""Principal coordinates of a cohort's samples over their KR distances, no device: the rule of include/epik_amd.h restated
here in numpy (the Jacobi rounds are test_epca_cpu's) against epik_amd_cohort_pcoa_host and _pcoa_kr_host -- every byte of
mu, coord and the info block --, the star whose eigenvalues are known by hand, points in the plane, the sign and order
conventions, the C ABI's refusals, the drivers' and the launcher's flags, the file and the stand-alone host binary (plain
and under ASan + UBSan).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from epik_amd import capi, cohort as cohort_mod, synth
from test_capi_cpu import _header_symbols
from test_cohort_cpu import host_bins, numpy_first, numpy_kr, random_cells, same_bits  # noqa: F401 (host_bins: a fixture)
from test_epca_cpu import numpy_jacobi, sequential_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MAX_SWEEPS = 64


# ---- the rule, restated ----------------------------------------------------------------------------------------------
def numpy_centred(kr, totals):
    """(used, B [L][L], scale, trace) of the rule: the squares, Gower's centring, every sum a chain from +0.0."""
    kr = np.asarray(kr, dtype=np.float64)
    used = np.flatnonzero(np.asarray(totals) > 0)
    count = len(used)
    d = kr[np.ix_(used, used)]
    a2 = d * d
    if not count:
        return used, np.zeros((0, 0)), np.float64(0.0), np.float64(0.0)
    r = sequential_sum(a2.T, 1) / np.float64(count)                             # (r_i walks KR[u_j][u_i], as the header says)
    g = sequential_sum(r, 0) / np.float64(count)
    b = -0.5 * (((a2 - r[:, None]) - r[None, :]) + g)
    upper = np.arange(count)[:, None] <= np.arange(count)[None, :]
    b = np.where(upper, b, b.T)                                                 # i <= j by the rule, the rest its mirror
    diag = b.diagonal().copy()
    return used, b, np.float64(np.abs(diag).max()), np.float64(sequential_sum(diag, 0))


def numpy_decomposition(kr, totals):
    """(used, scale, trace, A, V, sweeps, converged) of the rule: everything that does not depend on K."""
    used, b, scale, trace = numpy_centred(kr, totals)
    return (used, scale, trace) + tuple(numpy_jacobi(b, scale))


def numpy_pcoa(kr, totals, num_components, decomposition=None):
    """(mu [S], coord [S][K], info) by the header's text."""
    s, k_all = len(totals), int(num_components)
    used, scale, trace, a, v, sweeps, converged = decomposition or numpy_decomposition(kr, totals)
    count = len(used)
    mu_all = a.diagonal().copy()
    order = np.lexsort((np.arange(count), -mu_all))                             # (mu descending, j ascending)
    kc = min(k_all, count)
    floor = 2.0 ** -40 * scale
    mu, coord = np.zeros(s), np.zeros((s, k_all))
    pos = neg = np.float64(0.0)
    for k in range(count):
        jk = order[k]
        mu[k] = mu_all[jk]
        if mu[k] > floor:
            pos = pos + mu[k]
        if mu[k] < -floor:
            neg = neg + mu[k]
        if k >= kc or not mu[k] > floor:
            continue
        column = v[:, jk]
        sign = -1.0 if column[np.argmax(np.abs(column))] < 0 else 1.0           # (argmax: the first of the largest)
        coord[used, k] = sign * (column * np.sqrt(mu[k]))
    info = np.zeros(1, dtype=capi.PCOA_INFO)
    info[0] = (count, kc, sweeps, converged, trace, scale, pos, neg)
    return mu, coord, info[0]


def host_pcoa_kr_raw(kr, totals, k):
    """(mu, coord, info) straight from the C entry, into poisoned buffers."""
    lib = capi.load()
    kr = np.ascontiguousarray(kr, dtype=np.float64)
    totals = np.ascontiguousarray(totals, dtype=U64)
    s = len(totals)
    mu, coord, info = np.zeros(s), np.zeros((s, k)), np.zeros(1, dtype=capi.PCOA_INFO)
    for buf in (mu, coord, info):
        buf.view(np.uint8)[:] = 0xA5
    assert lib.epik_amd_cohort_pcoa_kr_host(kr.ctypes.data, totals.ctypes.data, s, k, mu.ctypes.data, coord.ctypes.data,
                                            info.ctypes.data) == capi.OK, lib.epik_amd_last_error()
    return mu, coord, info[0]


def assert_pcoa(got, want, what=""):
    """Every byte of mu, coord and the info block; `got` and `want` are tuples or `cohort.Pcoa`."""
    parts = [(x.mu, x.coord, x.info) if isinstance(x, cohort_mod.Pcoa) else x for x in (got, want)]
    (mu, coord, info), (w_mu, w_coord, w_info) = parts
    assert np.asarray(info).tobytes() == np.asarray(w_info).tobytes(), (what, info, w_info)
    assert same_bits(mu, w_mu), (what, mu, w_mu)
    assert same_bits(coord, w_coord), (what, np.argwhere(np.asarray(coord).view(U64) != np.asarray(w_coord).view(U64))[:5])


PCOA_TREES = {}


def pcoa_tree(num_branches):
    """(first, branch_length) of a tree of 7 or 999 branches, some lengths 0."""
    if num_branches not in PCOA_TREES:
        tree = synth.make_tree((num_branches + 1) // 2, seed=31)
        bl = np.asarray(tree.branch_length, dtype=np.float64).copy()
        bl[::5] = 0.0
        assert len(tree.parent) == num_branches
        PCOA_TREES[num_branches] = (numpy_first(tree.parent), bl)
    return PCOA_TREES[num_branches]


def pcoa_cells(num_used, num_branches):
    """mass[S][N] with `num_used` samples of mass and one empty sample (sample 1, or the only one)."""
    rng = np.random.default_rng(4000 + 7 * num_used + num_branches)
    mass = random_cells(rng, num_used + 1, num_branches, bits=42)
    mass[mass.sum(axis=1, dtype=U64) == 0, 0] = 5          # (a row of zeros by chance would change L)
    mass[1 if num_used else 0] = 0
    assert int((mass.sum(axis=1, dtype=U64) > 0).sum()) == num_used
    return mass


RESTATED = {}


def restated(num_used, num_branches):
    """(mass, first, bl, kr, totals, {K: numpy_pcoa}) of a case, computed once and shared with the device tests."""
    key = (num_used, num_branches)
    if key not in RESTATED:
        first, bl = pcoa_tree(num_branches)
        mass = pcoa_cells(num_used, num_branches)
        kr = numpy_kr(mass, first, bl)
        totals = mass.sum(axis=1, dtype=U64)
        once = numpy_decomposition(kr, totals)                                   # (the sweeps are the slow part: once a case)
        RESTATED[key] = (mass, first, bl, kr, totals, {k: numpy_pcoa(kr, totals, k, once) for k in (1, 5, 64)})
    return RESTATED[key]


USED = (0, 1, 2, 3, 33, 64, 65)


@pytest.mark.parametrize("num_branches", [7, 999])
@pytest.mark.parametrize("num_used", USED)
def test_pcoa_host_equals_the_numpy_restatement_bit_for_bit(num_used, num_branches):
    mass, first, bl, kr, totals, wants = restated(num_used, num_branches)
    assert same_bits(cohort_mod.kr_host(mass, first, bl), kr)
    for k, want in wants.items():
        got = host_pcoa_kr_raw(kr, totals, k)
        assert int(got[2]["used"]) == num_used and int(got[2]["components"]) == min(k, num_used)
        assert_pcoa(got, want, (num_used, num_branches, k))
        assert int(got[2]["converged"]) == 1 and int(got[2]["sweeps"]) <= MAX_SWEEPS
    assert_pcoa(cohort_mod.pcoa_host(mass, first, bl, 5), wants[5])
    assert_pcoa(cohort_mod.pcoa_kr_host(kr, totals, 64), wants[64])


# ---- the star, by hand -----------------------------------------------------------------------------------------------------
# Three leaves of length 1 around a centre, a sample on each leaf and one at the centre: KR is 2 between two leaves and 1
# from a leaf to the centre.  A2 is 4 and 1; r_leaf = 9/4, r_centre = 3/4, g = 15/8; B has 21/16 on the leaves' diagonal,
# -11/16 between two leaves, 1/16 from a leaf to the centre and -3/16 at the centre: all exact in binary.  On the leaves'
# differences B acts as 21/16 + 11/16 = 2 (twice); on (leaves / sqrt 3, centre) it is [[-1/16, sqrt 3 / 16], [sqrt 3 / 16,
# -3/16]] with trace -1/4 and determinant 0: the eigenvalues are {2, 2, 0, -1/4} and negative = (1/4) / 4 = 1/16.
STAR_KR = np.array([[0, 2, 2, 1], [2, 0, 2, 1], [2, 2, 0, 1], [1, 1, 1, 0]], dtype=np.float64)
STAR_MU = np.array([2.0, 2.0, 0.0, -0.25])
# The largest |mu - numpy.linalg.eigh(B)| of the host mirror on this case, measured on the CPU: 6.67e-16 (3 ulp of 1.0; eigh
# and the Jacobi sweeps each leave errors of a few ulp of the largest eigenvalue).  The tolerance is 16 times that, the margin
# for another library behind eigh.
STAR_MEASURED = 6.67e-16
STAR_TOLERANCE = 16 * STAR_MEASURED


def test_the_star_has_the_eigenvalues_derived_by_hand():
    totals = np.ones(4, U64)
    used, b, scale, trace = numpy_centred(STAR_KR, totals)
    want_b = np.full((4, 4), -11 / 16)
    want_b[3, :] = want_b[:, 3] = 1 / 16
    np.fill_diagonal(want_b, [21 / 16, 21 / 16, 21 / 16, -3 / 16])
    assert same_bits(b, want_b) and scale == 21 / 16 and trace == 3.75
    got = cohort_mod.pcoa_kr_host(STAR_KR, totals, 4)
    assert_pcoa(got, numpy_pcoa(STAR_KR, totals, 4))
    deviation = np.abs(got.mu - np.linalg.eigh(b)[0][::-1]).max()
    print(f"star: the host mirror is within {deviation:.3e} of numpy.linalg.eigh, sweeps {int(got.info['sweeps'])}")
    assert deviation <= STAR_TOLERANCE
    assert (np.abs(got.mu - STAR_MU) <= STAR_TOLERANCE).all(), got.mu
    assert got.kinds() == ["real", "real", "null", "negative"] and got.components == 4
    assert abs(float(got.info["pos"]) - 4.0) <= 2 * STAR_TOLERANCE and abs(float(got.info["neg"]) + 0.25) <= STAR_TOLERANCE
    assert abs(got.negative - 0.0625) <= STAR_TOLERANCE
    # the null and the negative axis carry no coordinates; the two real ones reproduce the leaves' triangle of side 2
    assert not got.coord[:, 2:].view(U64).any()
    xy = got.coord[:, :2]
    side = np.sqrt(((xy[:3, None, :] - xy[None, :3, :]) ** 2).sum(axis=2))
    assert (np.abs(side - STAR_KR[:3, :3]) <= 8 * STAR_TOLERANCE).all()
    assert (np.abs(xy[3]) <= 8 * STAR_TOLERANCE).all()      # the centre sits at the centroid of the real plane


# ---- points in the plane ---------------------------------------------------------------------------------------------------
# The largest |mu - eigh| of the host mirror on the 12 points, relative to the largest eigenvalue, measured on the CPU:
# 1.05e-15; 16 times that is the tolerance, as for the star.
PLANE_MEASURED = 1.05e-15
PLANE_TOLERANCE = 16 * PLANE_MEASURED


def plane_points():
    rng = np.random.default_rng(12)
    return rng.integers(-64, 65, size=(12, 2)).astype(np.float64) / 8.0        # (exact in binary)


def test_twelve_points_in_the_plane_come_back():
    xy = plane_points()
    dist = np.sqrt(((xy[:, None, :] - xy[None, :, :]) ** 2).sum(axis=2))
    totals = np.ones(12, U64)
    got = cohort_mod.pcoa_kr_host(dist, totals, 5)
    assert_pcoa(got, numpy_pcoa(dist, totals, 5))
    _, b, scale, _ = numpy_centred(dist, totals)
    top = float(got.mu[0])
    deviation = np.abs(got.mu - np.linalg.eigh(b)[0][::-1]).max() / top
    print(f"plane: the host mirror is within {deviation:.3e} of numpy.linalg.eigh (relative to mu_1), sweeps {int(got.info['sweeps'])}")
    assert deviation <= PLANE_TOLERANCE
    kinds = got.kinds()
    assert kinds[:2] == ["real", "real"] and "real" not in kinds[2:], kinds
    assert not got.coord[:, 2:].view(U64).any()
    back = np.sqrt(((got.coord[:, None, :2] - got.coord[None, :, :2]) ** 2).sum(axis=2))
    # a coordinate is v * sqrt(mu): an error of tolerance * mu_1 in B moves a distance by at most that over the distance scale
    assert (np.abs(back - dist) <= PLANE_TOLERANCE * top / np.sqrt(float(got.mu[1]))).all(), np.abs(back - dist).max()
    assert abs(got.negative) <= PLANE_TOLERANCE and abs(float(got.info["pos"]) - float(got.info["trace"])) <= PLANE_TOLERANCE * top


def test_a_forged_matrix_that_is_not_symmetric_reads_the_elements_the_header_names():
    """r_i from KR[u_j][u_i], B[i][j] for i <= j from KR[u_i][u_j]: the mirror and the restatement read what the device reads."""
    rng = np.random.default_rng(3)
    forged = rng.integers(1, 64, size=(9, 9)).astype(np.float64) / 8.0
    np.fill_diagonal(forged, 0.0)
    assert not np.array_equal(forged, forged.T)
    totals = np.array([1, 1, 0, 1, 1, 1, 1, 0, 1], U64)
    assert_pcoa(host_pcoa_kr_raw(forged, totals, 5), numpy_pcoa(forged, totals, 5))
    _, b, _, _ = numpy_centred(forged, totals)
    _, b_sym, _, _ = numpy_centred(np.triu(forged) + np.triu(forged).T, totals)
    assert not same_bits(b, b_sym)                              # the lower triangle does reach the row means


# ---- conventions -----------------------------------------------------------------------------------------------------------
def test_sign_order_and_the_cells_of_unused_samples():
    mass, first, bl, kr, totals, wants = restated(33, 7)
    mu, coord, info = wants[64]
    count, kc = 33, 33
    assert (np.diff(mu[:count]) <= 0).all() and not mu[count:].view(U64).any()          # descending, +0.0 beyond L
    floor = 2.0 ** -40 * float(info["scale"])
    assert (mu[:count] < -floor).any(), "the KR distance of a random cohort is not Euclidean"
    used = np.flatnonzero(totals > 0)
    for k in range(kc):
        column = coord[used, k]
        if mu[k] > floor:
            assert column[np.argmax(np.abs(column))] > 0, k                              # the largest coordinate is positive
        else:
            assert not column.view(U64).any(), k
    assert not coord[totals == 0].view(U64).any()
    # K beyond L: +0.0; K below L: the leading columns of the same decomposition
    assert not coord[:, kc:].view(U64).any()
    assert same_bits(wants[5][1], coord[:, :5]) and same_bits(wants[5][0], mu)
    # two samples: one axis, the two points half the distance from the origin each (d^2 / 2 is the eigenvalue)
    two = np.array([[0.0, 3.0], [3.0, 0.0]])
    got = cohort_mod.pcoa_kr_host(two, np.ones(2, U64), 2)
    ulp = 2.0 ** -52     # (one rotation by pi / 4: c = s = sqrt(1 / 2) rounded, so a few ulp of the values, no more)
    assert abs(got.mu[0] - 4.5) <= 4 * 4.5 * ulp and abs(got.mu[1]) <= 4 * 4.5 * ulp and got.kinds() == ["real", "null"]
    assert (np.abs(got.coord - [[1.5, 0.0], [-1.5, 0.0]]) <= 4 * 1.5 * ulp).all() and not got.coord[:, 1].view(U64).any()
    # identical samples: nothing to draw
    got = cohort_mod.pcoa_kr_host(np.zeros((3, 3)), np.ones(3, U64), 2)
    assert not got.coord.view(U64).any() and got.negative == 0.0 and got.kinds() == ["null"] * 3


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_pcoa_symbols_exist_and_refuse_what_the_header_says():
    lib = capi.load()
    names = ("epik_amd_cohort_pcoa_device", "epik_amd_cohort_pcoa", "epik_amd_cohort_pcoa_host", "epik_amd_cohort_pcoa_kr_host")
    for name in names:
        assert name in capi.EXPORTS and hasattr(lib, name)
    assert sorted(capi.EXPORTS) == _header_symbols() and capi.ABI_VERSION == 3 and capi.PCOA_INFO.itemsize == 48
    fields = ("used", "components", "sweeps", "converged", "trace", "scale", "pos", "neg")
    assert [capi.PCOA_INFO.fields[k][1] for k in fields] == [0, 4, 8, 12, 16, 24, 32, 40]
    err = lambda: lib.epik_amd_last_error().decode()
    info = np.zeros(1, dtype=capi.PCOA_INFO)
    assert lib.epik_amd_cohort_pcoa_device(None, None, 5, None, None, None, None) == capi.ERR_INVALID and "null cohort" in err()
    assert lib.epik_amd_cohort_pcoa(None, None, None, 5, None, None, info.ctypes.data) == capi.ERR_INVALID and "null cohort" in err()
    totals, mu, coord = np.ones(4, U64), np.zeros(4), np.zeros((4, 64))
    host = lib.epik_amd_cohort_pcoa_kr_host
    args = lambda d=STAR_KR, t=totals, s=4, k=2, a=mu, c=coord, i=info: (
        d.ctypes.data if d is not None else None, t.ctypes.data if t is not None else None, s, k,
        *(x.ctypes.data if x is not None else None for x in (a, c, i)))
    assert host(*args()) == capi.OK and int(info[0]["used"]) == 4 and int(info[0]["components"]) == 2
    assert host(*args(k=64)) == capi.OK and int(info[0]["components"]) == 4
    for bad in (0, 65, 0xFFFFFFFF):
        assert host(*args(k=bad)) == capi.ERR_INVALID and "num_components" in err() and "[1, 64]" in err()
    assert host(*args(s=0)) == capi.ERR_INVALID and "num_samples is 0" in err()
    for missing in ("d", "t", "a", "c", "i"):
        assert host(*args(**{missing: None})) == capi.ERR_INVALID and "null argument" in err(), missing
    first = cohort_mod.first_of([2, 2, -1])
    mass, bl = np.ones((2, 3), U64), np.ones(3)
    assert cohort_mod.pcoa_host(mass, first, bl, 2).components == 2
    for bad in (0, 65):
        with pytest.raises(capi.EpikAmdError):
            cohort_mod.pcoa_host(mass, first, bl, bad)
    with pytest.raises(capi.EpikAmdError):
        cohort_mod.pcoa_host(mass, np.array([0, 2, 0], dtype=np.uint32), bl, 2)      # first[1] above its branch
    with pytest.raises(ValueError):
        cohort_mod.pcoa_host(mass, first[:2], bl, 5)
    with pytest.raises(ValueError):
        cohort_mod.pcoa_kr_host(STAR_KR, totals[:3], 5)


# ---- the drivers and the launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", ["epik-dna", "epik-aa"])
def test_drivers_refuse_pcoa_without_cohort_and_name_the_flag(host_bins, tmp_path, binary):
    base = [os.path.join(host_bins, binary), "-d", str(tmp_path / "none.ekdb"), "-q", str(tmp_path / "none.list"), "-o", str(tmp_path)]
    for extra, flag, needs in ((["--cohort-pcoa"], "--cohort-pcoa", "--cohort "),
                               (["--cohort-pcoa", "--cohort-pcoa-components", "3"], "--cohort-pcoa", "--cohort "),
                               (["--cohort", "--cohort-pcoa-components", "3"], "--cohort-pcoa-components", "--cohort-pcoa "),
                               (["--cohort", "--cohort-pcoa", "--cohort-pcoa-components", "0"], "--cohort-pcoa-components", "[1, 64]"),
                               (["--cohort", "--cohort-pcoa", "--cohort-pcoa-components", "65"], "--cohort-pcoa-components", "[1, 64]"),
                               (["--cohort", "--cohort-pcoa", "--cohort-pcoa-components", "x"], "--cohort-pcoa-components", "[1, 64]")):
        run = subprocess.run(base + extra, capture_output=True, text=True)
        assert run.returncode == 255, run.stdout + run.stderr
        assert run.stderr.startswith("Error:") and flag in run.stderr and needs in run.stderr, (extra, run.stderr)
        assert "Loading database" not in run.stdout and "HIP device" not in run.stderr and not list(tmp_path.iterdir())
    out = subprocess.run([os.path.join(host_bins, binary), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-pcoa " in out.stdout and "--cohort-pcoa-components" in out.stdout
    assert "cohort_pcoa_<list>.tsv" in out.stdout


def test_launcher_passes_the_flags_only_when_given():
    import click
    import epik
    kw = dict(database="db.ekdb", states="nucl", omega=1.5, mu=1.0, outputdir="out", threads=1, max_ram="", gpus=1,
              input_file="samples.list")
    default = epik.driver_command(**kw)
    assert "--cohort-pcoa" not in " ".join(default)
    assert epik.driver_command(**kw, cohort_pcoa=False, cohort_pcoa_components=None) == default
    assert "--cohort-pcoa" not in " ".join(epik.driver_command(**kw, cohort=True))
    assert epik.driver_command(**kw, cohort=True, cohort_pcoa=True)[:-1] == default[:-1] + ["--cohort", "--cohort-pcoa"]
    assert epik.driver_command(**kw, cohort=True, cohort_pcoa=True, cohort_pcoa_components=3)[:-1] == \
        default[:-1] + ["--cohort", "--cohort-pcoa", "--cohort-pcoa-components", "3"]
    # beside the other analyses of a cohort, and with --strand and --taxonomy
    both = epik.driver_command(**kw, cohort=True, cohort_pcoa=True, cohort_epca=True, cohort_permanova="f.tsv", strand="both",
                               taxonomy="t.tsv")
    assert all(flag in both for flag in ("--cohort-pcoa", "--cohort-epca", "--cohort-permanova", "--strand", "--taxonomy"))
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort_pcoa=True)
    with pytest.raises(click.UsageError):
        epik.driver_command(**kw, cohort=True, cohort_pcoa_components=3)
    me = os.path.join(ROOT, "epik.py")
    out = subprocess.run([sys.executable, me, "place", "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--cohort-pcoa" in out.stdout and "--cohort-pcoa-components" in out.stdout
    run = subprocess.run([sys.executable, me, "place", "-i", me, "-o", ROOT, "--cohort-pcoa", me], capture_output=True, text=True)
    assert run.returncode == 2 and "--cohort" in run.stderr, (run.stdout, run.stderr)


# ---- the file --------------------------------------------------------------------------------------------------------------
def test_the_file_reads_back_and_keeps_names(tmp_path):
    names = ["a", "skin 3", "it's", "none", "z.9_-"]
    totals = np.array([1, 1, 1, 0, 1], U64)
    kr = np.full((5, 5), -1.0)
    kr[np.ix_([0, 1, 2, 4], [0, 1, 2, 4])] = STAR_KR
    pcoa = cohort_mod.pcoa_kr_host(kr, totals, 3)
    text = cohort_mod.format_pcoa_tsv(names, totals, pcoa)
    lines = text.split("\n")
    assert lines[0] == (f"# epik_amd pcoa v1  samples=5 used=4 components=3 sweeps={int(pcoa.info['sweeps'])} converged=1 "
                        f"negative={'%.17g' % pcoa.negative}")
    assert lines[1] == "# unused\tnone"
    assert [ln.split("\t")[4] for ln in lines[2:6]] == ["real", "real", "null", "negative"]
    assert lines[2].split("\t")[:4] == ["# eigenvalue", "1", "%.17g" % pcoa.mu[0], "%.17g" % (pcoa.mu[0] / float(pcoa.info["pos"]))]
    assert lines[6] == "name\tpc1\tpc2\tpc3" and [ln.split("\t")[0] for ln in lines[7:11]] == ["a", "skin 3", "it's", "z.9_-"]
    assert len(lines) == 12 and lines[-1] == ""
    path = tmp_path / "cohort_pcoa_x.tsv"
    path.write_bytes(text.encode())
    back_names, coord, info = cohort_mod.read_pcoa_tsv(str(path))
    assert back_names == ["a", "skin 3", "it's", "z.9_-"] and info["unused"] == ["none"]
    assert same_bits(coord, pcoa.coord[totals > 0][:, :3]) and same_bits(info["mu"], pcoa.mu[:4])   # %.17g reads back to the same double
    assert (info["samples"], info["used"], info["components"], info["converged"]) == (5, 4, 3, 1)
    assert info["kind"] == pcoa.kinds() and info["negative"] == pcoa.negative
    path.write_text("# something else\n")
    with pytest.raises(ValueError):
        cohort_mod.read_pcoa_tsv(str(path))
    with pytest.raises(ValueError):
        cohort_mod.format_pcoa_tsv(names, np.ones(5, U64), pcoa)
    # nothing used: the first line, the unused samples, the column of names alone
    empty = cohort_mod.pcoa_kr_host(np.zeros((2, 2)), np.zeros(2, U64), 5)
    assert cohort_mod.format_pcoa_tsv(["x y", "q"], [0, 0], empty) == (
        "# epik_amd pcoa v1  samples=2 used=0 components=0 sweeps=1 converged=1 negative=0\n# unused\tx y\n# unused\tq\nname\n")


# ---- the host code stand-alone -----------------------------------------------------------------------------------------
def _kr_input(path, mass, first, bl):
    with open(path, "wb") as fh:
        fh.write(np.array(mass.shape, dtype="<u8").tobytes() + np.ascontiguousarray(mass, U64).tobytes() +
                 np.ascontiguousarray(first, np.uint32).tobytes() + np.ascontiguousarray(bl, np.float64).tobytes())


@pytest.mark.parametrize("sanitized", [False, True])
def test_host_test_binary_pcoa_is_the_library_s_and_writes_the_formatter_s_bytes(host_bins, tmp_path, sanitized):
    binary = os.path.join(host_bins, "cohort_test")
    if sanitized:     # a stand-alone program built with -fsanitize=address,undefined: nothing is preloaded
        subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host"), "sanitize-cohort"], check=True, stdout=subprocess.DEVNULL)
        binary = os.path.join(host_bins, "san", "cohort_test_asan")
    for num_used in (0, 1, 3, 33):
        mass, first, bl, kr, totals, wants = restated(num_used, 7)
        _kr_input(tmp_path / "in.bin", mass, first, bl)
        run = subprocess.run([binary, "pcoa", str(tmp_path / "out.bin"), str(tmp_path / "in.bin"), "5"], capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_used, run.stderr)
        mu, coord, info = wants[5]
        assert (tmp_path / "out.bin").read_bytes() == mu.tobytes() + coord.tobytes() + np.asarray(info).tobytes(), num_used
        names = [f"s {i}" for i in range(len(mass))]
        (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
        run = subprocess.run([binary, "pcoa-tsv", str(tmp_path / "out.tsv"), str(tmp_path / "in.bin"), str(tmp_path / "names.txt"), "5"],
                             capture_output=True, text=True)
        assert run.returncode == 0 and not run.stderr, (num_used, run.stderr)
        want = cohort_mod.format_pcoa_tsv(names, totals, cohort_mod.Pcoa(mu, coord, info))
        assert (tmp_path / "out.tsv").read_bytes() == want.encode(), num_used
    for bad in ("0", "65"):
        run = subprocess.run([binary, "pcoa", str(tmp_path / "o.bin"), str(tmp_path / "in.bin"), bad], capture_output=True, text=True)
        assert run.returncode == 1 and "num_components" in run.stderr
