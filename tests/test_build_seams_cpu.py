"""The database-building path at its seams, without a GPU: the cases that test_build_seams_gpu.py runs
through the device, each checked here first against the most independent expectation that is affordable -- a closed form
written in the test where the case is planted, build_numpy (whose frontier uses the exact bound, not the mirrors' margin)
otherwise -- and against the host mirror, so that every case is known to be non-vacuous and right in the mirror before a
device sees it.  Planted ghost nodes (k = 2, L = 2, letters outside two chosen sets at -inf) walk the paths of the merge
one by one; chunks above the caps of the grids (restated below from the kernels' sources) walk every grid-stride loop;
k = 15 and amino k = 7 over a full tile of 64 windows walk the deepest stack and the widest staging; N around powers of
two up to 2^32 - 1 with the highest key walks the packed word; workspaces chosen to the byte walk both ways a chunk is
found too large; log_thr = -inf, +0.0 and -0.0; and the two halves of the ancestral posteriors that the chunked device
output is compared with.  Every comparison is of bytes."""
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epik_amd import alphabet, ancestral, build, filters  # noqa: E402
from epik_amd.synth import PKDB_VALUE  # noqa: E402
from test_ancestral_cpu import CHUNKING_CASE as ANCESTRAL_CHUNKING_CASE  # noqa: E402
from test_ancestral_cpu import get_case as ancestral_case  # noqa: E402
from test_ancestral_cpu import host_of as ancestral_host_of  # noqa: E402
from test_dbbuild_cpu import everything_case, make_case, same_db, special_case  # noqa: E402
from test_filter_cpu import FINITE_THR, same_bytes  # noqa: E402

# the caps of the grids, restated from the sources: a change there fails the preconditions below, loudly
BUILD_UNITS_CAP = 1 << 20             # build_place.hip, launch_enumerate: at most 2^20 workgroups, a (ghost node, tile) each
BUILD_ELEMENTS_CAP = 16384 * 256      # build_place.hip, blocks_for: kMaxBlocks x kBlock threads, an element each
FILTER_TILES_CAP = 8192 * 4           # filter_place.hip, grid_for(tiles, 8192): kBlockWaves = 4 waves a block, a tile of 64 keys each
FILTER_TILE_KEYS = 64
TUPLE_BYTES = 40                      # build_place.hip, kTupleBytes
WORKSPACE_SLACK = 8 * 256             # build_place.hip, add_range: `slack`
TILE_WINDOWS, MAX_K = 64, 15          # build_place.hip, kTile; build.hpp, kBuildMaxK

Triple = namedtuple("Triple", "keys offsets values")   # what same_db compares


def words_of(db):
    """(key, branch) of every entry as one integer: the order of the builder's store."""
    key = np.repeat(db.keys.astype(np.int64), np.diff(db.offsets.astype(np.int64)))
    return (key << 32) | db.values["branch"].astype(np.int64)


def pairs_to_triple(pairs):
    """{(key, branch): score} -> the database that holds exactly those."""
    order = sorted(pairs)
    values = np.zeros(len(order), dtype=PKDB_VALUE)
    values["branch"] = [b for _, b in order]
    values["score"] = np.array([pairs[p] for p in order], dtype=np.float32)
    keys, counts = np.unique(np.array([k for k, _ in order], dtype=np.int64), return_counts=True)
    offsets = np.zeros(len(keys) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    return Triple(keys.astype(np.uint32), offsets, values)


def chain(terms):
    """((+0.0 + t_0) + t_1) + ... in float32: the rule's sum."""
    s = np.float32(0.0)
    for t in terms:
        s = np.float32(s + np.float32(t))
    return s


# ---- 1. planted ghost nodes -------------------------------------------------------------------------------------------

PLANT_THR = np.float32(-1e30)


def plant(ghosts):
    """[(branch, {letter: logp} of site 0, {letter: logp} of site 1)] -> (logp float32 [G][2][4], branch_of uint32 [G]):
    -inf outside the chosen letters, so that with k = 2 and log_thr = -1e30 a ghost node yields exactly A0 x A1."""
    logp = np.full((len(ghosts), 2, 4), -np.inf, dtype=np.float32)
    branch_of = np.zeros(len(ghosts), dtype=np.uint32)
    for g, (branch, a0, a1) in enumerate(ghosts):
        branch_of[g] = branch
        for site, letters in enumerate((a0, a1)):
            for c, value in letters.items():
                logp[g, site, c] = np.float32(value)
    return logp, branch_of


def joined(chunks):
    return np.concatenate([c[0] for c in chunks]), np.concatenate([c[1] for c in chunks])


def planted_expectation(ghosts):
    """(keys, offsets, values) of planted ghost nodes given as (logp [G][2][4], branch_of [G]): per ghost node the 16
    sums float32(float32(0 + l0) + l1), the finite ones kept, the best of every (key, branch)."""
    logp, branch_of = ghosts
    first = (np.float32(0.0) + logp[:, 0, :]).astype(np.float32)
    s = (first[:, :, None] + logp[:, 1, None, :]).astype(np.float32).reshape(logp.shape[0], 16)
    g, key = np.nonzero(np.isfinite(s))                                   # (key = 4 c0 + c1)
    score = s[g, key]
    word = (key.astype(np.int64) << 32) | branch_of[g].astype(np.int64)
    order = np.argsort(word, kind="stable")
    word, score = word[order], score[order]
    head = np.ones(word.shape[0], dtype=bool)
    head[1:] = word[1:] != word[:-1]
    if word.shape[0]:
        word, score = word[head], np.maximum.reduceat(score, np.flatnonzero(head))   # the best score of every (key, branch)
    values = np.zeros(word.shape[0], dtype=PKDB_VALUE)
    values["branch"] = word & 0xFFFFFFFF
    values["score"] = score
    keys, counts = np.unique(word >> 32, return_counts=True)
    offsets = np.zeros(keys.shape[0] + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts)
    return Triple(keys.astype(np.uint32), offsets, values)


def planted_host(num_branches, ghosts, num_threads=1):
    return build.build_host("nucl", 2, num_branches, ghosts[0], ghosts[1], log_thr=PLANT_THR, num_threads=num_threads)


def test_planted_expectation_by_hand():
    ghosts = plant([(3, {0: -0.5, 2: -1.25}, {1: -0.25}), (1, {2: -3.0}, {1: -0.5, 3: -0.125}), (3, {2: -1.0}, {1: -0.25})])
    want = pairs_to_triple({(1, 3): np.float32(-0.75), (9, 3): np.float32(-1.25), (9, 1): np.float32(-3.5), (11, 1): np.float32(-3.125)})
    same_db(planted_expectation(ghosts), want)
    same_db(planted_host(4, ghosts), want)
    same_db(build.build_numpy("nucl", 2, 4, *ghosts, log_thr=PLANT_THR), want)


# ---- 2. the paths of the merge, planted -------------------------------------------------------------------------------

MERGE_N = 6
_BASE = [(2, {1: -0.3, 2: -1.7}, {1: -0.9, 2: -2.3}), (3, {1: -0.6, 2: -1.1}, {1: -0.2, 2: -2.9})]   # keys 5, 6, 9, 10 on branches 2 and 3


def _single(key, branch, score):
    return (branch, {key // 4: score / 4}, {key % 4: score})


def _shifted(ghosts, by):
    return [(b, {c: v + by for c, v in a0.items()}, {c: v + by for c, v in a1.items()}) for b, a0, a1 in ghosts]


_STORE_SINGLES = [(k, b) for k in (2, 5, 9, 13) for b in (1, 4)]
_BETWEEN_SINGLES = [(2, 0), (2, 3), (3, 2), (5, 2), (7, 5), (9, 3), (11, 0), (13, 2), (13, 5)]

#: name -> the chunks of one builder, each a list of planted ghost nodes
MERGE_SCENARIOS = {
    "lower": [_BASE, _shifted(_BASE, -0.5)],
    "higher": [_BASE, [(2, {1: -0.2, 2: -2.0}, {1: -0.9, 2: -2.3}), _BASE[1]]],
    "below": [_BASE, [(5, {0: -0.4}, {0: -1.1, 1: -0.6}), (0, {1: -0.8}, {1: -0.2}), (1, {0: -1.0, 1: -0.7}, {1: -0.3})]],
    "above": [_BASE, [(0, {3: -0.4}, {3: -1.1, 2: -0.5}), (4, {2: -0.8}, {2: -0.2}), (5, {2: -1.0, 3: -0.1}, {2: -0.3})]],
    "interleaved": [[_single(k, b, -0.1 * (k + b + 1)) for k, b in _STORE_SINGLES],
                    [_single(k, b, -0.07 * (k + b + 1)) for k, b in _BETWEEN_SINGLES]],
    "other-branches": [_BASE, [(0,) + _BASE[0][1:], (5,) + _BASE[1][1:]]],
    "repeats": [_BASE, [(2, {1: -3.0}, {1: -0.5}), (2, {1: -0.05}, {1: -0.05}), (2, {1: -1.0}, {1: -0.5})],
                [(4, {1: -2.0}, {3: -0.5}), (4, {1: -0.15}, {3: -0.35}), (4, {1: -1.0}, {3: -0.5})],
                [(2, {1: -3.0}, {1: -0.5}), (2, {1: -0.3}, {1: -0.3}), (2, {1: -1.0}, {1: -0.5})]],
    "repeats-first": [[(2, {1: -3.0}, {1: -0.5}), (2, {1: -0.05}, {1: -0.05}), (2, {1: -1.0}, {1: -0.5})], _BASE],
    "empty": [_BASE, [], [(1, {}, {}), (4, {0: -0.5}, {})], [(0, {3: -0.4}, {3: -1.1, 0: -0.2})]],
}


def merge_chunks(name):
    return [plant(chunk) for chunk in MERGE_SCENARIOS[name]]


def merge_stages(name):
    """The planted expectation after every chunk of a scenario."""
    chunks = merge_chunks(name)
    return [planted_expectation(joined(chunks[:i + 1])) for i in range(len(chunks))]


def check_merge_path(name, stages):
    """What makes a scenario walk its path, asserted on the databases after every chunk."""
    words = [words_of(s) for s in stages]
    fresh = np.setdiff1d(words[1], words[0])
    if name == "lower":
        assert words[1].tobytes() == words[0].tobytes() and stages[1].values.tobytes() == stages[0].values.tobytes()
    elif name == "higher":
        raised = stages[1].values["score"] != stages[0].values["score"]
        assert len(fresh) == 0 and np.array_equal(words[1][raised], [(5 << 32) | 2, (6 << 32) | 2])
        assert np.all(stages[1].values["score"][raised] > stages[0].values["score"][raised])
        assert stages[1].values["score"][raised].tobytes() == np.array([chain([-0.2, -0.9]), chain([-0.2, -2.3])], np.float32).tobytes()
    elif name == "below":
        assert len(fresh) == 5 and len(words[1]) == len(words[0]) + 5 and fresh.max() < words[0].min()
        assert (fresh >> 32).max() == words[0].min() >> 32                     # (one of them on the first key's lower branch)
    elif name == "above":
        assert len(fresh) == 5 and len(words[1]) == len(words[0]) + 5 and fresh.min() > words[0].max()
        assert (fresh >> 32).min() == words[0].max() >> 32
    elif name == "interleaved":
        is_new = np.isin(words[1], fresh)
        assert len(fresh) == len(words[0]) + 1 and np.all(is_new[0::2]) and not np.any(is_new[1::2])
    elif name == "other-branches":
        assert np.array_equal(stages[1].keys, stages[0].keys) and len(fresh) == len(words[0])
        for i in range(len(stages[1].keys)):
            br = stages[1].values["branch"][int(stages[1].offsets[i]):int(stages[1].offsets[i + 1])]
            assert br.tolist() == [0, 2, 3, 5]
    elif name == "repeats":
        at = int(np.flatnonzero(words[1] == ((5 << 32) | 2))[0])
        assert len(fresh) == 0 and stages[1].values["score"][at] == chain([-0.05, -0.05]) > stages[0].values["score"][at]
        new = int(np.flatnonzero(words[2] == ((7 << 32) | 4))[0])
        assert len(words[2]) == len(words[1]) + 1 and stages[2].values["score"][new] == chain([-0.15, -0.35])
        assert stages[3].values.tobytes() == stages[2].values.tobytes()
    elif name == "repeats-first":
        assert len(words[0]) == 1 and stages[0].values["score"][0] == chain([-0.05, -0.05])
        assert stages[1].values["score"][int(np.flatnonzero(words[1] == words[0][0])[0])] == chain([-0.05, -0.05])
    elif name == "empty":
        assert len(words[0]) == 8 and stages[1].values.tobytes() == stages[0].values.tobytes() == stages[2].values.tobytes()
        assert len(words[3]) == 10


@pytest.mark.parametrize("name", sorted(MERGE_SCENARIOS))
def test_merge_scenarios_in_the_host_mirror(name):
    chunks, stages = merge_chunks(name), merge_stages(name)
    check_merge_path(name, stages)
    for i, want in enumerate(stages):
        sofar = joined(chunks[:i + 1])
        same_db(planted_host(MERGE_N, sofar), want)
        same_db(build.build_numpy("nucl", 2, MERGE_N, *sofar, log_thr=PLANT_THR), want)


# ---- 3. grid strides --------------------------------------------------------------------------------------------------

_ONCE = {}


def once(name, make):
    """A case or an expectation computed once and shared; treat as read-only."""
    if name not in _ONCE:
        _ONCE[name] = make()
    return _ONCE[name]


def _stride_build_case():
    rng = np.random.default_rng(2024)
    G = (1 << 20) + 300
    branch_of = rng.permutation(G).astype(np.uint32)
    logp = np.full((G, 2, 4), -np.inf, dtype=np.float32)
    logp[:, 0, :] = -(rng.random((G, 4), dtype=np.float32) * np.float32(4.0) + np.float32(0.01))
    last = rng.integers(0, 4, size=G)
    logp[np.arange(G), 1, last] = -(rng.random(G, dtype=np.float32) * np.float32(4.0) + np.float32(0.01))
    # the second chunk: 300 branches over the whole range; on the even ones two first letters score higher and two lower,
    # on the odd ones another last letter: four new pairs each
    home = np.empty(G, dtype=np.int64)
    home[branch_of] = np.arange(G)
    picked = home[np.linspace(0, G - 1, 300).astype(np.int64)]
    second = logp[picked].copy()
    second[0::2, 0, :2] *= np.float32(0.5)
    second[0::2, 0, 2:] *= np.float32(2.0)
    moved = second[1::2]
    was = last[picked[1::2]]
    rows = np.arange(moved.shape[0])
    scores = moved[rows, 1, was].copy()
    moved[rows, 1, was] = -np.inf
    moved[rows, 1, (was + 1) % 4] = scores
    second[1::2] = moved
    return dict(N=G, chunks=[(logp, branch_of), (second, branch_of[picked].copy())])


def stride_build_case():
    return once("stride-build", _stride_build_case)


def stride_build_stages():
    def make():
        chunks = stride_build_case()["chunks"]
        return [planted_expectation(chunks[0]), planted_expectation(joined(chunks))]
    return once("stride-build-stages", make)


def stride_build_host():
    case = stride_build_case()
    return once("stride-build-host", lambda: planted_host(case["N"], joined(case["chunks"]), num_threads=16))


def test_stride_build_case_is_above_every_cap_and_right_in_the_host_mirror():
    case, stages = stride_build_case(), stride_build_stages()
    first, second = case["chunks"]
    assert first[0].shape[0] * 1 > BUILD_UNITS_CAP                       # (L = k: one tile a ghost node)
    assert first[0].size > BUILD_ELEMENTS_CAP                            # validate_kernel
    assert len(stages[0].values) == 4 * first[0].shape[0] > BUILD_ELEMENTS_CAP   # head_flag, reduce, merge_write, csr
    assert len(stages[1].values) == len(stages[0].values) + 4 * 150
    words = [words_of(s) for s in stages]
    old = words[0][np.minimum(np.searchsorted(words[0], words[1]), len(words[0]) - 1)] == words[1]
    fresh = words[1][~old]
    assert len(fresh) == 600 and fresh.min() < words[0][len(words[0]) // 100] and fresh.max() > words[0][-len(words[0]) // 100]
    raised = stages[1].values["score"][old] != stages[0].values["score"]
    assert raised.sum() == 2 * 150 and np.all(stages[1].values["score"][old][raised] > stages[0].values["score"][raised])
    same_db(stride_build_host(), stages[1])


def _stride_filter_case():
    """K = 2^21 + 65 keys in the layout of test_filter_cpu.forge_lists, forged without a loop over the keys: nine in ten lists
    of one entry, the rest of 2 to 5, some 300 longer than 256; scores in [log_thr, -2] with ties.  The last 65 keys lie in
    the two tiles that only a second sweep of the grid reaches: they hold three long lists, and the smallest and the
    largest value of `best` and of `mif0`."""
    rng = np.random.default_rng(77)
    K, N, floor = (1 << 21) + 65, 400, float(FINITE_THR)
    second_sweep = FILTER_TILES_CAP * FILTER_TILE_KEYS
    lengths = np.ones(K, dtype=np.int64)
    some = np.flatnonzero(rng.random(K) < 0.1)
    lengths[some] = rng.integers(2, 6, size=len(some))
    long_at = np.concatenate([rng.choice(second_sweep, size=300, replace=False), [K - 60, K - 31, K - 2]])
    lengths[long_at] = rng.integers(257, 391, size=len(long_at))
    lengths[K - 2] = N
    lengths[[K - 50, K - 40]] = 1
    offsets = np.zeros(K + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    begin = offsets[:-1].astype(np.int64)
    E = int(offsets[-1])
    values = np.zeros(E, dtype=PKDB_VALUE)
    score = (np.float32(-2.0) + rng.random(E, dtype=np.float32) * np.float32(floor + 2.0)).astype(np.float32)
    pick = rng.random(E)
    score[pick < 0.2] = np.float32(-2.5)
    score[(pick >= 0.2) & (pick < 0.25)] = np.float32(floor)
    values["score"] = np.maximum(score, np.float32(floor))
    within = np.arange(E, dtype=np.int64) - np.repeat(begin, lengths)
    start, step = rng.integers(0, 160, size=K), rng.integers(1, 60, size=K)    # ascending distinct branches below 160 + 4 x 59
    values["branch"] = np.repeat(start, lengths) + within * np.repeat(step, lengths)
    for k in long_at:
        n = int(lengths[k])
        values["branch"][begin[k]:begin[k] + n] = np.sort(rng.choice(N, size=n, replace=False)) if n < N else np.arange(N)
    values["score"][begin[K - 50]] = np.float32(-0.5)                        # the smallest `best` but one
    values["score"][begin[K - 40]] = np.float32(0.0)                         # the smallest `best` and the smallest `mif0`
    values["score"][begin[K - 2]:begin[K - 2] + N] = -np.inf                 # Z = 0: the largest of both
    keys = (np.arange(K, dtype=np.uint64) * 5 + 2).astype(np.uint32)
    return dict(N=N, log_thr=FINITE_THR, keys=keys, offsets=offsets, values=values, second_sweep=second_sweep, long_at=long_at)


def stride_filter_case():
    return once("stride-filter", _stride_filter_case)


def stride_filter_host(name):
    def make():
        c = stride_filter_case()
        return filters.rank_host(c["N"], c["log_thr"], c["keys"], c["offsets"], c["values"], name, seed=9, num_threads=16)
    return once("stride-filter-host-" + name, make)


def image_of(value):
    bits = value.view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits | np.uint64(1 << 63))


def test_stride_filter_case_needs_a_second_sweep_for_its_bit_range():
    c = stride_filter_case()
    K, edge = len(c["keys"]), c["second_sweep"]
    tiles = (K + FILTER_TILE_KEYS - 1) // FILTER_TILE_KEYS
    assert tiles > FILTER_TILES_CAP and K - edge == 65
    lengths = np.diff(c["offsets"].astype(np.int64))
    assert (lengths == 1).mean() > 0.88 and (lengths[c["long_at"]] > 256).all() and (c["long_at"] >= edge).sum() == 3
    assert np.all(np.diff(c["values"]["branch"].astype(np.int64))[np.diff(np.repeat(np.arange(K), lengths)) == 0] > 0)
    assert c["values"]["branch"].max() < c["N"]
    for name in ("best", "mif0"):
        value, order = stride_filter_host(name)
        image = image_of(value)
        assert image.argmin() >= edge and image.argmax() >= edge, name
        assert image[edge:].min() < image[:edge].min() and image[edge:].max() > image[:edge].max(), name
        first_range = int(image[:edge].min() ^ image[:edge].max()).bit_length()
        assert first_range < int(image.min() ^ image.max()).bit_length(), name   # the sorted bits depend on the second sweep
        assert order[-1] == K - 2, name
    assert stride_filter_host("best")[1][1] == K - 50 and stride_filter_host("best")[1][0] == K - 40
    small = slice(edge - 3 * FILTER_TILE_KEYS, K)                               # the numpy restatement on the seam's own keys
    lo, hi = int(c["offsets"][small.start]), int(c["offsets"][-1])
    part = (c["keys"][small], c["offsets"][small.start:] - np.uint64(lo), c["values"][lo:hi])
    for name in filters.FILTERS:
        want = filters.rank_numpy(c["N"], c["log_thr"], *part, name, seed=9)
        assert same_bytes(filters.rank_host(c["N"], c["log_thr"], *part, name, seed=9), want), name
        assert stride_filter_host(name)[0][small].tobytes() == want[0].tobytes(), name


# ---- 4. the deepest and widest walks ----------------------------------------------------------------------------------

#: name -> (states, k, L, G, N, seed, log_thr); log_thr chosen with build_numpy so that 10^4 <= entries <= 2 10^6
DEEP_CASES = {
    "nucl-k15-L15-G1": ("nucl", 15, 15, 1, 5, 3101, -5.6),
    "nucl-k15-L16-G3": ("nucl", 15, 16, 3, 9, 3102, -5.0),
    "nucl-k15-L78-G2": ("nucl", 15, 78, 2, 300, 3103, -3.9),
    "nucl-k15-L79-G2": ("nucl", 15, 79, 2, 70000, 3104, -3.9),
    "amino-k7-L70-G2": ("amino", 7, 70, 2, 7, 3105, -4.2),
    "amino-k7-L71-G2": ("amino", 7, 71, 2, 33, 3106, -4.2),
}
DEEP_ROUNDING_THR = np.float32(-0.75)


def deep_case(name):
    states, k, L, G, N, seed, log_thr = DEEP_CASES[name]
    case = make_case(states, k, L, G, N, seed=seed, kind="spread")      # (top = 0.9)
    case["log_thr"] = np.float32(log_thr)
    return case


def deep_rounding_case():
    """Random float32 logp at k = 15 (not the logarithm of anything): sums that depend on the order of the additions."""
    rng = np.random.default_rng(19)
    logp = (-rng.random((2, 30, 4)) * rng.choice([0.02, 0.3, 3.0], size=(2, 30, 4))).astype(np.float32)
    return dict(states="nucl", k=15, N=5, logp=logp, branch_of=np.array([4, 0], dtype=np.uint32), log_thr=DEEP_ROUNDING_THR)


def numpy_of(case):
    return build.build_numpy(case["states"], case["k"], case["N"], case["logp"], case["branch_of"], log_thr=case["log_thr"])


def host_of(case, **kw):
    return build.build_host(case["states"], case["k"], case["N"], case["logp"], case["branch_of"], log_thr=case["log_thr"], **kw)


def deep_expectation(name):
    return once("deep-" + name, lambda: numpy_of(deep_case(name)))


def check_best_kmers(case, db):
    """Without the mirrors: the best k-mer of every window is there on its branch with the left-to-right sum, and nothing
    lies below log_thr."""
    logp, k = case["logp"], case["k"]
    sigma = logp.shape[2]
    want = {}
    for g in range(logp.shape[0]):
        letters, best = logp[g].argmax(axis=1), logp[g].max(axis=1)
        for w in range(logp.shape[1] - k + 1):
            key = 0
            for c in letters[w:w + k]:
                key = key * sigma + int(c)
            pair = (key, int(case["branch_of"][g]))
            want[pair] = max(want.get(pair, np.float32(-np.inf)), chain(best[w:w + k]))
    words = words_of(db)
    for (key, branch), score in want.items():
        assert score >= case["log_thr"]
        at = int(np.searchsorted(words, (key << 32) | branch))
        assert at < len(words) and words[at] == (key << 32) | branch, "the best k-mer of a window is missing"
        assert db.values["score"][at].tobytes() == score.tobytes()
    assert np.all(db.values["score"] >= case["log_thr"])


@pytest.mark.parametrize("name", sorted(DEEP_CASES))
def test_deep_cases_in_the_host_mirror(name):
    case, want = deep_case(name), deep_expectation(name)
    assert 10 ** 4 <= want.num_entries <= 2 * 10 ** 6, want.num_entries
    W = case["logp"].shape[1] - case["k"] + 1
    if "L78" in name or "L70" in name:
        assert W == TILE_WINDOWS                                          # one full tile
    if "L78" in name:
        assert TILE_WINDOWS + case["k"] - 1 == TILE_WINDOWS + MAX_K - 1  # rows == kMaxRows
    if "L79" in name or "L71" in name:
        assert W == TILE_WINDOWS + 1                                      # a second tile of one window
    check_best_kmers(case, want)
    same_db(host_of(case, num_threads=4), want)


def deep_rounding_thresholds():
    """(base, the bits of its lowest stored score, one step towards 0)."""
    def make():
        base = numpy_of(deep_rounding_case())
        lowest = base.values["score"].min()
        return base, np.float32(lowest), np.nextafter(np.float32(lowest), np.float32(0))
    return once("deep-rounding", make)


def test_deep_rounding_and_the_threshold_seam_in_the_host_mirror():
    case = deep_rounding_case()
    base, at, above = deep_rounding_thresholds()
    assert 10 ** 4 <= base.num_entries <= 2 * 10 ** 6, base.num_entries
    logp, k = case["logp"], case["k"]
    best = logp[0].max(axis=1)
    W = logp.shape[1] - k + 1
    left = np.array([chain(best[w:w + k]) for w in range(W)], dtype=np.float32)
    right = np.array([chain(best[w:w + k][::-1]) for w in range(W)], dtype=np.float32)
    assert np.any(left.view(np.uint32) != right.view(np.uint32)), "the two orders agree: the case is vacuous"
    same_db(host_of(case), base)
    lowest = np.flatnonzero(base.values["score"] == at)
    case["log_thr"] = at
    kept = host_of(case)
    same_db(kept, numpy_of(case))
    same_db(kept, base)
    case["log_thr"] = above
    dropped = host_of(case)
    same_db(dropped, numpy_of(case))
    assert dropped.num_entries == base.num_entries - len(lowest) and dropped.values.tobytes() == np.delete(base.values, lowest).tobytes()


# ---- 5. the width of the packed word ----------------------------------------------------------------------------------

WIDTH_N = [1, 2, 3, 4, 5, 255, 256, 257, 65536, 65537, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]
WIDTH_ALPHABETS = [("nucl", 15), ("amino", 7)]


def width_case(states, k, N):
    """Three ghost nodes of one window: all sites one-hot on letter 0 (key 0, +0.0) on branch 0; on the last letter (key
    sigma^k - 1, +0.0) on branch N - 1; one-hot on a pattern, three of its sites with two finite letters (8 keys in
    between) on branch N / 2.  Returns (case, the closed-form expectation)."""
    sigma = alphabet.alphabet_size(states)
    logp = np.full((3, k, sigma), -np.inf, dtype=np.float32)
    logp[0, :, 0] = 0.0
    logp[1, :, sigma - 1] = 0.0
    pattern = [(7 * j + 1) % sigma for j in range(k)]
    logp[2, np.arange(k), pattern] = 0.0
    two = {0: -0.3, k // 2: -0.7, k - 1: -0.2}                        # site -> the logp of the pattern's letter there
    other = {j: ((pattern[j] + 2) % sigma, np.float32(-1.1 - 0.1 * j)) for j in two}
    for j, value in two.items():
        logp[2, j, pattern[j]] = np.float32(value)
        logp[2, j, other[j][0]] = other[j][1]
    branches = [0, N - 1, N // 2 if N > 2 else N - 1]
    pairs = {}

    def put(key, branch, score):
        pairs[(key, branch)] = max(pairs.get((key, branch), np.float32(-np.inf)), score)

    put(0, branches[0], np.float32(0.0))
    put(sigma ** k - 1, branches[1], np.float32(0.0))
    sites = sorted(two)
    for choice in range(8):
        letters, terms = list(pattern), [np.float32(0.0)] * k
        for bit, j in enumerate(sites):
            if choice >> bit & 1:
                letters[j], terms[j] = other[j]
            else:
                terms[j] = np.float32(two[j])
        key = 0
        for c in letters:
            key = key * sigma + c
        put(key, branches[2], chain(terms))
    case = dict(states=states, k=k, N=N, logp=logp, branch_of=np.array(branches, dtype=np.uint32), log_thr=None)
    return case, pairs_to_triple(pairs)


@pytest.mark.parametrize("N", WIDTH_N)
@pytest.mark.parametrize("states,k", WIDTH_ALPHABETS)
def test_width_cases_in_the_host_mirror(states, k, N):
    case, want = width_case(states, k, N)
    sigma = alphabet.alphabet_size(states)
    assert want.keys[0] == 0 and want.keys[-1] == sigma ** k - 1 and len(want.keys) == 10 and len(want.values) == 10
    assert want.values["branch"][-1] == N - 1 and want.values["branch"][0] == 0 and want.values["score"].view(np.uint32)[0] == 0
    db = host_of(case)
    same_db(db, want)
    for name in ("best", "mif0"):
        ranked = filters.rank_host(N, db.log_threshold, db.keys, db.offsets, db.values, name)
        assert same_bytes(ranked, filters.rank_numpy(N, db.log_threshold, db.keys, db.offsets, db.values, name)), name


# ---- 6. workspaces, splits and the partial add -------------------------------------------------------------------------

def item_bytes(case, ghosts=None):
    """build_place.hip, add_range: align_up((items + 1) * 8) with items = G W sigma, to 256 bytes."""
    G, L, sigma = case["logp"].shape
    items = (G if ghosts is None else ghosts) * (L - case["k"] + 1) * sigma
    return ((items + 1) * 8 + 255) // 256 * 256


def finite_tuples(case, ghosts=None):
    """The k-mers of a chunk without a -inf letter, window by window: what survives log_thr = -1e30."""
    finite = np.isfinite(case["logp"]).sum(axis=2).astype(np.int64)
    k, total = case["k"], 0
    for g in (range(finite.shape[0]) if ghosts is None else ghosts):
        total += sum(int(np.prod(finite[g, w:w + k])) for w in range(finite.shape[1] - k + 1))
    return total


def items_route_case():
    """Uniform posteriors under omega = 2 (0.25 a letter against 0.5 a letter: nothing survives) but for five stretches of
    eight sites at 0.97 on one letter, 43 k-mers each: a chunk whose items do not fit a workspace of 20 000 bytes though
    its tuples are few."""
    rng = np.random.default_rng(61)
    p = np.full((16, 40, 4), 0.25, dtype=np.float32)
    for g in (0, 3, 7, 8, 15):
        at = int(rng.integers(0, 32))
        p[g, at:at + 8] = 0.01
        p[g, np.arange(at, at + 8), rng.integers(0, 4, size=8)] = 0.97
    case = dict(states="nucl", k=6, N=9, logp=build.logp_from_posteriors(p), branch_of=rng.integers(0, 9, size=16).astype(np.uint32),
                log_thr=build.default_log_thr("nucl", 6, 2.0))
    return case, 20000


def tuples_route_case():
    """`everything`: 520 items and some 400 000 tuples (a few posteriors print as 0); 12 MB hold the items and one ghost
    node's tuples, not both's."""
    return everything_case(), 12 << 20


def refusal_cases():
    """route -> (a chunk of one ghost node, a workspace it is refused with, the bytes the refusal must name)."""
    lonely = np.full((1, 300, 4), -np.inf, dtype=np.float32)
    lonely[0, 150, 2], lonely[0, 151, 1] = -0.5, -0.25                   # one survivor: what a workspace of exactly X holds
    items = dict(states="nucl", k=2, N=3, logp=lonely, branch_of=np.array([1], dtype=np.uint32), log_thr=PLANT_THR)
    whole = everything_case()
    tuples = dict(whole, logp=whole["logp"][:1], branch_of=whole["branch_of"][:1])
    return {"items": (items, 4096, 2 * item_bytes(items) + WORKSPACE_SLACK + TUPLE_BYTES),
            "tuples": (tuples, 1 << 20, 2 * item_bytes(tuples) + WORKSPACE_SLACK + finite_tuples(tuples) * TUPLE_BYTES)}


def partial_case():
    """Four ghost nodes under log_thr = -1e30: 0, 1 and 3 one-hot but for two sites (a handful of k-mers a window), 2 the
    first ghost node of `everything` (some 200 000 k-mers).  4 MB hold 0 and 1 together but not 2."""
    rng = np.random.default_rng(62)
    whole = everything_case()
    logp = np.full((4, 70, 4), -np.inf, dtype=np.float32)
    for g in (0, 1, 3):
        logp[g, np.arange(70), rng.integers(0, 4, size=70)] = -(rng.random(70) * 0.3).astype(np.float32)
        logp[g, [20, 45], :] = -(rng.random((2, 4)) * 2).astype(np.float32)
    logp[2] = whole["logp"][0]
    return dict(states="nucl", k=6, N=5, logp=logp, branch_of=np.array([4, 0, 2, 4], dtype=np.uint32), log_thr=np.float32(-1e30)), 4 << 20


def sliced(case, ghosts):
    ghosts = list(ghosts)
    return dict(case, logp=np.ascontiguousarray(case["logp"][ghosts]), branch_of=np.ascontiguousarray(case["branch_of"][ghosts]))


def test_workspace_cases_take_the_routes_they_are_named_for():
    case, ws = items_route_case()
    need = 2 * item_bytes(case) + WORKSPACE_SLACK + TUPLE_BYTES
    assert ws < 2 * item_bytes(case) and need > ws                        # the items alone: found before the count
    db = numpy_of(case)
    assert 100 < db.num_entries <= 5 * 43
    same_db(host_of(case), db)
    case, ws = tuples_route_case()
    db = host_of(case)
    one = max(finite_tuples(case, [0]), finite_tuples(case, [1]))          # the tuples of one ghost node
    assert 2 * item_bytes(case) + WORKSPACE_SLACK + TUPLE_BYTES <= ws < 2 * item_bytes(case) + WORKSPACE_SLACK + finite_tuples(case) * TUPLE_BYTES
    assert ws >= 2 * item_bytes(case, 1) + WORKSPACE_SLACK + one * TUPLE_BYTES and db.num_entries == 2 * 4096 and one > 150000
    same_db(db, numpy_of(case))
    for route, (chunk, ws, need) in refusal_cases().items():
        db = numpy_of(chunk)
        same_db(host_of(chunk), db)
        assert ws < need and db.num_entries == {"items": 1, "tuples": 4096}[route]
        first_way = 2 * item_bytes(chunk) + WORKSPACE_SLACK + TUPLE_BYTES
        assert (ws < first_way) == (route == "items")
    case, ws = partial_case()
    tuples = [int((np.isfinite(case["logp"][g]).sum(axis=1) > 1).sum()) for g in range(4)]
    assert tuples[2] >= 60 and max(tuples[0], tuples[1], tuples[3]) == 2
    heavy = 2 * item_bytes(case, 1) + WORKSPACE_SLACK + finite_tuples(case, [2]) * TUPLE_BYTES
    light = 2 * item_bytes(case, 2) + WORKSPACE_SLACK + finite_tuples(case, [0, 1]) * TUPLE_BYTES
    assert light <= ws < heavy
    for ghosts in ((0, 1), (0, 1, 3)):
        part = sliced(case, ghosts)
        same_db(host_of(part), numpy_of(part))
        assert 0 < numpy_of(part).num_entries <= len(ghosts) * 65 * 16


# ---- 7. log_thr at its ends -------------------------------------------------------------------------------------------

def log_thr_case(log_thr):
    """`special` of test_dbbuild_cpu.py under another threshold.  For -inf its first 14 sites only, three ordinary ones on
    either side of the nine with p = 1: over all 40 sites every k-mer is met somewhere with a finite score, and a
    (key, branch) keeps its best."""
    case = special_case()
    case["log_thr"] = np.float32(log_thr)
    if np.isneginf(log_thr):
        case["logp"] = np.ascontiguousarray(case["logp"][:, :14])
    return case


def test_log_thr_minus_infinity_in_the_host_mirror():
    case = log_thr_case(-np.inf)
    assert np.isneginf(case["logp"][:, 3:12]).sum() == 3 * 9 * 3 and case["logp"].shape[1] == 14
    db = host_of(case)
    same_db(db, numpy_of(case))
    assert np.isneginf(db.values["score"]).any() and (db.values["score"].view(np.uint32) == 0).any()
    assert np.array_equal(db.keys, np.arange(4 ** 4, dtype=np.uint32))     # every k-mer passes -inf >= -inf
    for name in filters.FILTERS:
        ranked = filters.rank_host(case["N"], db.log_threshold, db.keys, db.offsets, db.values, name, seed=3)
        assert same_bytes(ranked, filters.rank_numpy(case["N"], db.log_threshold, db.keys, db.offsets, db.values, name, seed=3)), name


def test_log_thr_of_either_zero_in_the_host_mirror():
    plus, minus = host_of(log_thr_case(0.0)), host_of(log_thr_case(-0.0))
    assert np.signbit(log_thr_case(-0.0)["log_thr"]) and not np.signbit(log_thr_case(0.0)["log_thr"])
    same_db(plus, minus)
    same_db(plus, numpy_of(log_thr_case(0.0)))
    same_db(minus, numpy_of(log_thr_case(-0.0)))
    assert plus.num_entries > 0 and np.all(plus.values["score"].view(np.uint32) == 0)


# ---- 8. the halves of the ancestral posteriors --------------------------------------------------------------------------

ANCESTRAL_SEAM_CASES = (ANCESTRAL_CHUNKING_CASE, "tile-L%d" % (ancestral.TILE_SITES + 1))
ANCESTRAL_CHUNK_SITES = (1, 5, 64, 65)


def ancestral_want(name, ghosts):
    """(post, branch_of, dead) of the host mirror for one choice of ghost nodes, computed once."""
    if ghosts == "both":
        return ancestral_host_of(name)
    case = ancestral_case(name)
    return once(f"ancestral-{name}-{ghosts}", lambda: ancestral.posteriors_host(*case["inputs"], case["masks"], ghosts, num_threads=4))


@pytest.mark.parametrize("name", ANCESTRAL_SEAM_CASES)
def test_inner_and_outer_are_the_halves_of_both(name):
    both, inner, outer = (ancestral_want(name, g) for g in ("both", "inner", "outer"))
    half = both[0].shape[0] // 2
    assert inner[0].tobytes() == both[0][:half].tobytes() and outer[0].tobytes() == both[0][half:].tobytes()
    assert inner[0].tobytes() != outer[0].tobytes() and inner[2] + outer[2] == both[2]
    assert np.array_equal(inner[1], both[1][:half]) and np.array_equal(outer[1], both[1][half:])
    L = ancestral_case(name)["masks"].shape[1]
    assert L > max(ANCESTRAL_CHUNK_SITES[:2]) and L >= ANCESTRAL_CHUNK_SITES[-1]    # several chunks, and one that is the whole
