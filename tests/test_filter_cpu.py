"""Ranking phylo-k-mers by informativeness without a device (include/epik_amd.h, "Ranking phylo-k-mers by
informativeness"): ek_exp2 and ek_log2 of the library against their numpy restatement bit for bit and against numpy's own
exp2 and log2; hand-derived values; the host mirror's bytes against the restatement's on forged databases; `best` against
the order dbfile has always written; the loaders' cut of a file written in a given order; the launcher's flags; the host
code stand-alone under the sanitizers."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from click.testing import CliRunner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epik_amd import capi, dbfile, filters, synth  # noqa: E402
from epik_amd.synth import PKDB_VALUE  # noqa: E402

EPIK_PY = os.path.join(ROOT, "epik.py")
BIN = os.path.join(ROOT, "epik_amd", "bin")
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
BRANCH_COUNTS = (1, 3, 65, 1303)
FINITE_THR = np.float32(-3.6123599)     # log10((1.5 / 4)^k) at k = 8, about


def same_bytes(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype


def load_epik_py():
    import importlib.util
    spec = importlib.util.spec_from_file_location("epik_launcher", EPIK_PY)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


# ---- forged databases, shared with test_filter_gpu.py ----------------------------------------------------------------

def forge_lists(lengths, num_branches, log_thr, rng, key_step=5):
    """A CSR database with lists of the given lengths (cut at N): random scores in [log_thr, 0] (or [-6, 0]), a share of
    them exactly at log_thr, at 0 and at -inf; ascending distinct branches; keys ascending with gaps."""
    N = int(num_branches)
    lens = np.minimum(np.asarray(lengths, dtype=np.int64), N)
    K = len(lens)
    offsets = np.zeros(K + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    E = int(offsets[-1])
    floor = float(log_thr) if np.isfinite(log_thr) else -6.0
    values = np.zeros(E, dtype=PKDB_VALUE)
    values["score"] = (rng.random(E) * floor).astype(np.float32)
    pick = rng.random(E)
    values["score"][pick < 0.04] = 0.0
    values["score"][(pick >= 0.04) & (pick < 0.08)] = -np.inf
    values["score"][(pick >= 0.08) & (pick < 0.12)] = np.float32(floor)
    begin = offsets[:-1].astype(np.int64)
    for b, n in zip(begin, lens):
        values["branch"][b:b + n] = np.sort(rng.choice(N, size=int(n), replace=False)) if n < N else np.arange(N)
    keys = (np.arange(K, dtype=np.uint64) * key_step + 2).astype(np.uint32)
    return keys, offsets, values


def forged_case(num_branches, log_thr, seed=0, repeats=2):
    """Every length of LENGTHS and N itself, `repeats` times over, then a key whose Z is 0 when log_thr is -inf (all its
    entries at -inf) and a copy of the first list on other branches (a tie in mif0 and best)."""
    rng = np.random.default_rng(1000 * seed + num_branches)
    lengths = list((LENGTHS + (num_branches,)) * repeats) + [min(3, num_branches), 1]
    keys, offsets, values = forge_lists(lengths, num_branches, log_thr, rng)
    dead = slice(int(offsets[-3]), int(offsets[-2]))
    values["score"][dead] = -np.inf
    values["score"][int(offsets[-2])] = values["score"][0]
    values["branch"][int(offsets[-2])] = num_branches - 1
    return keys, offsets, values


_cases = {}


def get_forged(num_branches, log_thr):
    key = (num_branches, float(log_thr))
    if key not in _cases:
        _cases[key] = forged_case(num_branches, log_thr)
        for array in _cases[key]:
            array.setflags(write=False)
    return _cases[key]


# ---- the two functions -------------------------------------------------------------------------------------------------

def exp2_grid():
    rng = np.random.default_rng(5)
    scores = np.concatenate([-(rng.random(40000) * 12).astype(np.float32), np.float32(-np.arange(0, 400) / 8)])
    return np.concatenate([
        [0.0, -0.0, -0.5, -1.5, -2.5, -3.5, -1021.5, -1022.0, np.nextafter(-1022.0, -np.inf), -1022.5, -1023.0, -1074.0, -1075.0, -2000.0,
         -1e300, -np.inf],
        scores.astype(np.float64) * filters.LOG2_10,
        -rng.random(40000) * 1022, -np.arange(0, 1023, dtype=np.float64), -np.arange(0, 1022, dtype=np.float64) - 0.5,
        np.nextafter(-np.arange(0, 1022, dtype=np.float64) - 0.5, 0), np.nextafter(-np.arange(0, 1022, dtype=np.float64) - 0.5, -np.inf),
    ])


def log2_grid():
    rng = np.random.default_rng(6)
    powers = 2.0 ** np.arange(-1022, 1024)
    seam = math.sqrt(0.5) * 2.0 ** np.arange(-1021, 1023)
    return np.concatenate([
        powers, seam, np.nextafter(seam, 0), np.nextafter(seam, np.inf), np.nextafter(np.nextafter(seam, 0), 0),
        np.nextafter(powers, np.inf), np.nextafter(powers[1:], 0),
        rng.random(40000) * 1303, 1.0 + (rng.random(20000) - 0.5) * 1e-6, 2.0 ** rng.uniform(-1022, 1023, size=40000),
    ])


def test_math_functions_equal_the_numpy_restatement_bit_for_bit():
    x = exp2_grid()
    got, _ = filters.math_host(x)
    assert got.tobytes() == filters.ek_exp2(x).tobytes()
    assert not np.signbit(got[x < -1022]).any() and (got[x < -1022] == 0).all()       # +0.0 below -1022, -inf included
    assert got[0] == 1.0 and got[1] == 1.0 and got[7] == 2.0 ** -1022
    z = log2_grid()
    _, got = filters.math_host(z)
    assert got.tobytes() == filters.ek_log2(z).tobytes()
    assert np.array_equal(got[:2046], np.arange(-1022, 1024, dtype=np.float64))       # the powers of two are exact
    edge = np.array([0.0, np.inf, -1.0])
    _, got = filters.math_host(edge)
    assert got[0] == -np.inf and got[1] == np.inf and np.isnan(got[2]) and np.isnan(filters.ek_log2(edge)[2])


def test_math_functions_stay_close_to_numpy_s():
    """Within 2^-40 relative of numpy's exp2 and log2 (absolute for |log2| below 1).  Measured here: exp2 1.0 x 2^-52,
    log2 2.3e-16 relative."""
    x = exp2_grid()
    x = x[x >= -1022]                    # below, the rule gives +0.0 where libm gives a subnormal
    got, _ = filters.math_host(x)
    want = np.exp2(x)
    worst = float(np.max(np.abs(got - want) / want))
    print(f"ek_exp2: max relative error against numpy {worst:.3e} = {worst * 2 ** 52:.3f} x 2^-52")
    assert worst <= 2.0 ** -40
    z = log2_grid()
    _, got = filters.math_host(z)
    want = np.log2(z)
    worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    print(f"ek_log2: max error against numpy, relative to max(|log2 z|, 1): {worst:.3e}")
    assert worst <= 2.0 ** -40


# ---- hand-derived values ---------------------------------------------------------------------------------------------------

def one_key(scores, branches=None):
    values = np.zeros(len(scores), dtype=PKDB_VALUE)
    values["score"] = scores
    values["branch"] = np.arange(len(scores)) if branches is None else branches
    return np.array([9], np.uint32), np.array([0, len(scores)], np.uint64), values


@pytest.mark.parametrize("rank", [filters.rank_numpy, filters.rank_host], ids=["numpy", "host"])
def test_hand_derived_values(rank):
    for N, s in ((8, -2.5), (65, -0.75), (1303, -3.0), (2, 0.0)):
        value, order = rank(N, FINITE_THR, *one_key(np.full(N, s, np.float32)), "mif0")
        assert abs(value[0] - math.log2(N)) <= 1e-12 and order.tolist() == [0]      # all N branches at one score: log2 N
    value, _ = rank(1, FINITE_THR, *one_key(np.float32([-1.25])), "mif0")
    assert abs(value[0]) <= 1e-12                                                      # N = 1: nothing to be unsure of
    value, _ = rank(1, FINITE_THR, *one_key(np.float32([0.0])), "mif0")
    assert value[0] == 0.0 and not np.signbit(value[0])
    for N, thr in ((5, np.float32(-1.0)), (1303, FINITE_THR), (3, np.float32(-0.5))):
        value, _ = rank(N, thr, *one_key(np.float32([0.0]), [N - 1]), "mif0")          # one entry at p = 1, N - 1 at t
        t = 10.0 ** float(thr)
        Z = 1.0 + (N - 1) * t
        assert abs(value[0] - (math.log2(Z) - (N - 1) * t * math.log2(t) / Z)) <= 1e-12
    # two keys with the same multiset of scores on other branches: one value, ordered by key; a sharper key comes first
    scores = np.float32([-0.3, -2.0, -1.1, -0.3, -2.0, -1.1, -0.01])
    values = np.zeros(7, dtype=PKDB_VALUE)
    values["score"] = scores
    values["branch"] = [1, 4, 6, 0, 2, 5, 3]
    value, order = rank(7, np.float32(-3.0), np.array([3, 11, 40], np.uint32), np.array([0, 3, 6, 7], np.uint64), values, "mif0")
    assert value[0] == value[1] and value[2] < value[0] and order.tolist() == [2, 0, 1]
    # Z = 0: +inf, ranked last; -inf entries beside a live one add nothing
    values = np.zeros(5, dtype=PKDB_VALUE)
    values["score"] = [-np.inf, -np.inf, -1.0, -np.inf, -1.0]
    values["branch"] = [0, 1, 0, 1, 2]
    value, order = rank(4, np.float32(-np.inf), np.array([1, 2, 3], np.uint32), np.array([0, 2, 4, 5], np.uint64), values, "mif0")
    assert value[0] == np.inf and value[1] == value[2] and abs(value[1]) <= 1e-12 and order.tolist() == [1, 2, 0]
    assert not np.isnan(value).any()


# ---- the host mirror against the restatement ---------------------------------------------------------------------------

@pytest.mark.parametrize("log_thr", [FINITE_THR, np.float32(-np.inf)], ids=["thr", "thr-inf"])
@pytest.mark.parametrize("num_branches", BRANCH_COUNTS)
def test_host_mirror_equals_the_numpy_restatement(num_branches, log_thr):
    keys, offsets, values = get_forged(num_branches, log_thr)
    assert set(np.diff(offsets.astype(np.int64)).tolist()) >= {min(n, num_branches) for n in LENGTHS + (num_branches,)}
    for name in filters.FILTERS:
        want = filters.rank_numpy(num_branches, log_thr, keys, offsets, values, name, seed=77)
        assert not np.isnan(want[0]).any() and sorted(want[1].tolist()) == list(range(len(keys)))
        for threads in (1, 16):
            assert same_bytes(filters.rank_host(num_branches, log_thr, keys, offsets, values, name, seed=77, num_threads=threads), want), \
                (name, threads)
    if not np.isfinite(log_thr):
        value, order = filters.rank_numpy(num_branches, log_thr, keys, offsets, values, "mif0")
        assert value[len(keys) - 2] == np.inf and order[-1] == len(keys) - 2            # the key with Z = 0


def test_host_mirror_threads_over_many_keys():
    """More keys than one thread's share, so that sorted runs are merged: 1 and 16 threads, the same bytes as numpy."""
    rng = np.random.default_rng(8)
    keys, offsets, values = forge_lists(rng.integers(1, 4, size=70000), 40, FINITE_THR, rng)
    values["score"][rng.random(len(values)) < 0.5] = np.float32(-1.5)                   # many ties
    for name in filters.FILTERS:
        want = filters.rank_numpy(40, FINITE_THR, keys, offsets, values, name, seed=3)
        for threads in (1, 16):
            assert same_bytes(filters.rank_host(40, FINITE_THR, keys, offsets, values, name, seed=3, num_threads=threads), want)


@pytest.mark.parametrize("name", filters.FILTERS)
def test_no_key_and_one_key(name):
    empty = (np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, PKDB_VALUE))
    for rank in (filters.rank_numpy, filters.rank_host):
        value, order = rank(5, FINITE_THR, *empty, name)
        assert value.shape == (0,) and order.shape == (0,) and value.dtype == np.float64 and order.dtype == np.uint32
    single = one_key(np.float32([-0.5, -1.0]))
    assert same_bytes(filters.rank_host(5, FINITE_THR, *single, name, seed=2), filters.rank_numpy(5, FINITE_THR, *single, name, seed=2))


def test_random_is_the_mix_of_seed_and_key():
    keys, offsets, values = get_forged(65, FINITE_THR)
    a, order_a = filters.rank_host(65, FINITE_THR, keys, offsets, values, "random", seed=1)
    b, order_b = filters.rank_host(65, FINITE_THR, keys, offsets, values, "random", seed=2)
    assert not np.array_equal(order_a, order_b) and (a < 2.0 ** 53).all() and (a == np.floor(a)).all()
    z = (1 + int(keys[4]) * 0x9E3779B97F4A7C15) % 2 ** 64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert a[4] == float((z ^ (z >> 31)) >> 11)


def sparse_of(db):
    lens = np.diff(db.offsets.astype(np.int64))
    keys = np.flatnonzero(lens)
    offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens[keys])
    return keys.astype(np.uint32), offsets


@pytest.mark.parametrize("tied", [False, True], ids=["random", "tied"])
def test_best_is_the_order_written_so_far(tied):
    tree = synth.make_tree(30, seed=2)
    db = synth.make_db(tree.num_nodes, kmer_size=5, seed=9, p_present=0.6)
    if tied:
        db.values["score"][:] = np.round(db.values["score"] * 2) / 2     # few different scores: many ties
        db.values["score"][::7] = -0.0
    keys, offsets = sparse_of(db)
    for rank in (filters.rank_numpy, filters.rank_host):
        _, order = rank(db.num_branches, db.log_threshold, keys, offsets, db.values, "best")
        assert np.array_equal(keys[order].astype(np.int64), dbfile.informativeness_order(db.offsets, db.values))


# ---- files ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_bins():
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "csrc")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", os.path.join(ROOT, "epik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    return BIN


def small_sparse_db():
    tree = synth.make_tree(12, seed=4)
    dense = synth.make_db(tree.num_nodes, kmer_size=4, seed=6, p_present=0.7, lognormal=(1.0, 1.0))
    keys, offsets = sparse_of(dense)
    db = synth.SynthDB(states="nucl", kmer_size=4, omega=1.5, num_branches=tree.num_nodes, offsets=offsets, values=dense.values, keys=keys)
    return tree, dense, db


def test_write_db_order_none_is_unchanged_and_order_is_honoured(tmp_path):
    tree, dense, db = small_sparse_db()
    a, b, c = (str(tmp_path / name) for name in ("dense.ekdb", "sparse.ekdb", "explicit.ekdb"))
    dbfile.write_db(a, dense, tree.newick())
    dbfile.write_db(b, db, tree.newick())
    _, best = filters.rank_host(db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, "best")
    dbfile.write_db(c, db, tree.newick(), order=best)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read() == open(c, "rb").read()
    # ... and those bytes are the records one by one, as write_db assembled them before
    import struct
    import zlib
    at = 8 + 16 + 24 + len(tree.newick())
    crc = 0
    for key in dbfile.informativeness_order(dense.offsets, dense.values):
        lo, hi = int(dense.offsets[key]), int(dense.offsets[key + 1])
        record = struct.pack("<II", int(key), hi - lo) + dense.values[lo:hi].tobytes()
        assert raw[at:at + len(record)] == record
        at += len(record)
        crc = zlib.crc32(record, crc)
    assert raw[at:] == dbfile.END_MAGIC + struct.pack("<QQII", len(db.keys), db.num_entries, crc & 0xFFFFFFFF, 0)
    with pytest.raises(ValueError, match="different indices"):
        dbfile.write_db(c, db, tree.newick(), order=np.zeros(len(db.keys), np.uint32))


@pytest.mark.parametrize("name", ["mif0", "random"])
def test_loaders_cut_a_prefix_of_the_given_order(host_bins, tmp_path, name):
    tree, _, db = small_sparse_db()
    _, order = filters.rank_host(db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, name, seed=5)
    assert not np.array_equal(order, filters.rank_host(db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, "best")[1])
    path = str(tmp_path / "ranked.ekdb")
    dbfile.write_db(path, db, tree.newick(), order=order)
    K = len(db.keys)
    first_half = set(int(k) for k in db.keys[order[:math.ceil(K / 2)]])
    got, _ = dbfile.read_db(path, mu=0.5)
    assert set(np.flatnonzero(np.diff(got.offsets.astype(np.int64))).tolist()) == first_half
    whole, _ = dbfile.read_db(path)
    assert whole.values.tobytes() == db.values.tobytes()
    out = subprocess.run([os.path.join(host_bins, "host_test"), "load", path, str(2 ** 62), "0", "1", "0.5"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    line = [x for x in out.stdout.splitlines() if x.startswith("keys")][0]
    assert set(int(x) for x in line.split()[1:]) == first_half


# ---- the library's refusals ------------------------------------------------------------------------------------------------

def test_host_entry_refusals():
    keys, offsets, values = (a.copy() for a in get_forged(65, FINITE_THR))

    def refused(message, **kw):
        args = dict(num_branches=65, log_thr=FINITE_THR, keys=keys, offsets=offsets, values=values, filter=1)
        args.update(kw)
        with pytest.raises(capi.EpikAmdError, match=message) as info:
            filters.rank_host(**args)
        assert info.value.code == capi.ERR_INVALID

    refused("unknown filter 3", filter=3)
    bad = values.copy()
    bad["score"][40] = np.nan
    bad["score"][90] = 0.25
    bad["branch"][7] = 65
    refused(r"values\[40\]\.score = nan is a NaN or above 0", values=bad)
    bad["score"][40] = -1.0
    refused(r"values\[90\]\.score = 0\.25 is a NaN or above 0", values=bad, filter=0)
    bad["score"][90] = -1.0
    refused(r"values\[7\]\.branch = 65 is not below num_branches = 65", values=bad, filter=2)
    wrong = offsets.copy()
    wrong[9] = wrong[8] - 1
    refused(r"offsets\[9\] = \d+ is below offsets\[8\]", offsets=wrong)
    refused("num_branches must be at least 1", num_branches=0)
    refused("log_thr = 0.5 must be at most 0", log_thr=np.float32(0.5))
    with pytest.raises(ValueError, match="unknown filter 'mif1'"):
        filters.rank_host(65, FINITE_THR, keys, offsets, values, "mif1")
    for rank_numpy_refuses in ((dict(values=bad, offsets=wrong)), (dict(filter=7))):
        with pytest.raises(ValueError):
            args = dict(num_branches=65, log_thr=FINITE_THR, keys=keys, offsets=offsets, values=values, filter="mif0")
            args.update(rank_numpy_refuses)
            filters.rank_numpy(**args)
    lib = capi.load()
    for symbol in ("epik_amd_filter_rank_device", "epik_amd_filter_rank", "epik_amd_builder_rank", "epik_amd_filter_rank_host",
                   "epik_amd_filter_math_host"):
        assert hasattr(lib, symbol) and symbol in capi.EXPORTS
    assert filters.FILTERS == ("best", "mif0", "random")


def test_builder_of_the_host_mirror_ranks_on_the_host():
    import ctypes

    from epik_amd import build
    rng = np.random.default_rng(3)
    post = rng.dirichlet(np.full(4, 0.3), size=(10, 30)).astype(np.float32)
    logp, branch_of = build.logp_from_posteriors(post), rng.integers(0, 7, size=10).astype(np.uint32)
    db = build.build_host("nucl", 5, 7, logp, branch_of, omega=1.5)
    lib = capi.load()
    handle = ctypes.c_void_p()
    capi.check(lib.epik_amd_build_host(4, 5, 7, ctypes.c_float(float(db.log_threshold)), logp.ctypes.data, branch_of.ctypes.data, 10, 30, 1,
                                       ctypes.byref(handle)))
    try:
        K = len(db.keys)
        for fid, name in enumerate(filters.FILTERS):
            value, order = np.zeros(K, np.float64), np.zeros(K, np.uint32)
            capi.check(lib.epik_amd_builder_rank(handle, fid, 11, value.ctypes.data, order.ctypes.data))
            assert same_bytes((value, order), filters.rank_numpy(7, db.log_threshold, db.keys, db.offsets, db.values, name, seed=11))
        assert lib.epik_amd_builder_rank(handle, 9, 0, value.ctypes.data, order.ctypes.data) == capi.ERR_INVALID
    finally:
        lib.epik_amd_builder_destroy(handle)


# ---- the launcher ------------------------------------------------------------------------------------------------------------

def test_launcher_lists_rank_and_refuses_bad_filters(tmp_path):
    launcher = load_epik_py()
    runner = CliRunner()
    listed = runner.invoke(launcher.epik, ["--help"])
    assert listed.exit_code == 0 and "rank" in listed.output and "reconstruct" in listed.output
    assert sorted(launcher.epik.commands) == ["build", "extend", "place"]
    for command in ("build", "reconstruct", "rank"):
        text = runner.invoke(launcher.epik, [command, "--help"]).output
        assert "--filter" in text and "--filter-seed" in text
    missing = str(tmp_path / "nothing")           # the refusals come before any file is opened
    build = ["build", "-t", missing, "--ar-probs", missing, "--ar-tree", missing, "-k", "6", "-o", str(tmp_path / "o.ekdb")]
    reconstruct = ["reconstruct", "-t", missing, "-r", missing, "--model", "JC", "-k", "6", "-o", str(tmp_path / "o.ekdb")]
    rank = ["rank", "-i", missing, "-o", str(tmp_path / "o.ekdb")]
    for argv in (build, reconstruct, rank):
        run = runner.invoke(launcher.epik, argv + ["--filter", "mif1"])
        assert run.exit_code == 2 and "--filter: 'mif1' is no filter (one of best, mif0, random)" in run.output
        extra = ["--filter", "mif0"] if argv is rank else []
        run = runner.invoke(launcher.epik, argv + extra + ["--filter-seed", "4"])
        assert run.exit_code == 2 and "--filter-seed needs --filter random" in run.output
        run = runner.invoke(launcher.epik, argv + ["--filter", "random", "--filter-seed", "4"])
        assert run.exit_code == 2 and "does not exist" in run.output
    assert not os.path.exists(str(tmp_path / "o.ekdb"))


def test_rank_command_on_the_host(tmp_path):
    """`epik.py rank --host`: best -> mif0 -> best gives the first file's bytes back; mu = 0.5 of the mif0 file holds the first
    half of rank_numpy's order."""
    tree, _, db = small_sparse_db()
    first, ranked, back = (str(tmp_path / name) for name in ("best.ekdb", "mif0.ekdb", "back.ekdb"))
    dbfile.write_db(first, db, tree.newick())
    launcher = load_epik_py()
    runner = CliRunner()
    run = runner.invoke(launcher.epik, ["rank", "-i", first, "--filter", "mif0", "--host", "-o", ranked])
    assert run.exit_code == 0, run.output
    assert f"{len(db.keys)} k-mers, {db.num_entries} phylo-k-mers ranked by mif0" in run.output
    run = runner.invoke(launcher.epik, ["rank", "-i", ranked, "--filter", "best", "--host", "--threads", "3", "-o", back])
    assert run.exit_code == 0, run.output
    assert open(back, "rb").read() == open(first, "rb").read() != open(ranked, "rb").read()
    _, order = filters.rank_numpy(db.num_branches, db.log_threshold, db.keys, db.offsets, db.values, "mif0")
    want = str(tmp_path / "want.ekdb")
    dbfile.write_db(want, db, tree.newick(), order=order)
    assert open(want, "rb").read() == open(ranked, "rb").read()
    run = runner.invoke(launcher.epik, ["rank", "-i", EPIK_PY, "--filter", "mif0", "--host", "-o", back])
    assert run.exit_code == 2 and "is not an EPIKAMD1 file" in run.output


# ---- the host code stand-alone ---------------------------------------------------------------------------------------------

def test_host_code_under_sanitizers():
    """A stand-alone program over filter.cpp built with -fsanitize=address,undefined: the math functions at their edges, hand
    cases, a forged database on one thread and five, the refusals.  Nothing is preloaded."""
    host = os.path.join(ROOT, "epik_amd", "host")
    subprocess.run(["make", "-C", host, os.path.join(BIN, "filter_test"), "sanitize-filter"], check=True, stdout=subprocess.DEVNULL)
    for binary in (os.path.join(BIN, "filter_test"), os.path.join(BIN, "san", "filter_test_asan")):
        run = subprocess.run([binary], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and "filter selftest ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
