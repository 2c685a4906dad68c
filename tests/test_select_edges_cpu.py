"""Top-k selection, the ratio filter and the team merge on planted corrected scores: the scenes of test_select_edges_gpu.py,
and the proof -- on the CPU oracle and a numpy restatement of the selection's bookkeeping alone -- that every scene reaches the
seam it is named for.

Every placement ends in select_best_placements, sum_scores and filter_by_ratio (place_device.hpp, place_epilogue_body; the
slice epilogues of the team kernels; team_epilogue.hpp over the touched quads; the four forms of the merge).  That step
changes its path with the NUMBER OF CANDIDATES, and the candidates are not the best rows but every row that reaches tau, a
lower bound of the n_sel-th largest of the 64 per-lane maxima.  The random databases of the other tests have a dozen
candidates a read, no two equal scores, and their best rows spread evenly over the lanes.

A scene plants corrected scores exactly.  A read of exactly k letters has one k-mer; a row of its list gets count 1 and the
corrected score s / k, and with k = 4 that division is exact: order, ties and the unit spacing of the planted float32 values
survive it.  The same postings under k = 5 have rounded quotients (neighbours may collapse into a tie); the oracle is the
reference either way, but a scene's named seam is asserted for k = 4 only -- for k = 5 the restatement is held to the oracle
and what the scene reaches is listed.  Reads of two and three k-mers over lists that overlap in part give rows of mixed
counts and exact ties between rows reached through different lists.  Two databases have k = 6: there, and not with k = 4 or 5,
tiny numerators exist whose quotient the kernels' three-instruction division misses (`fast_division_differs`).

The restatement (`select_model`, `slice_models`, `merge_form`) is written from the code:

* lane l owns rows 4 l .. 4 l + 3 of every trip of 256 rows (load_trip / load_rows: i0 = base + 4 * lane), rows counted
  from the slice's first row in a team kernel;
* the touched-quad epilogue lists the touched quads of a slice in the order (trip of 64 16-byte vectors, quad within the
  vector, lane) -- list_touched_quads -- and entry i of that list belongs to lane i % 64;
* n_sel = min(keep, touched); tau = ord(v) & ~255 for v the n_sel-th largest lane maximum, 1 when fewer than n_sel lanes
  hold an edge (every edge is a candidate); `tau_search` replays the bit search with its two shortcuts literally and every
  scene asserts that it equals the closed form;
* n_cand = number of edges with ord(score) >= tau; the one-wavefront kernel ranks up to 64 candidates out of the lanes, up
  to 128 and 192 with two and three keys a lane from LDS broadcasts, more by repeated selection; a slice holds 60;
* the merge takes M = slices * keep slots: four reads a wave up to 16, two up to 32, a slot a lane up to 64, a loop beyond.
"""
import numpy as np
import pytest

from epik_amd.synth import PKDB_VALUE, SynthDB, pack_reads

F32 = np.float32
WAVE_CAP, SLICE_CAP, TAU_STOP = 192, 60, 8      # kChunkCap, kTeamCandCap, EPIK_AMD_TAU_STOP
KEEPS = (1, 2, 7, 63, 64)
FACTORS = (0.0, 0.01, 1.0, float(np.finfo(np.float64).max))   # 1.0 still keeps the best row and its ties; create() takes any double
WAVE_N, TEAM_N = 600, {8: 136, 4: 260, 2: 260}
QUAD_N = 2100                                    # team2-sparse: slices of 1 050 rows hold 257 touched quads
QUAD_COUNTS = (1, 63, 64, 65, 128, 129, 192, 193, 256, 257)
# (layout, keep) of the GPU file's team cases: M = 16, 18, 20, 32, 36, 64, 66, 72 and the usual 7
TEAM_LAYOUTS = {"team2": 2, "team4": 4, "team8": 8, "team4x2": 8, "team4-classic": 4, "team4-sparse": 4, "team4-dense": 4,
                "team4-block2": 4}
TEAM_KEEPS = {2: (8, 9, 33, 64), 4: (4, 5, 8, 9, 16, 64), 8: (4, 8, 9)}


# ---- float32 in steps of a unit in the last place ---------------------------------------------------------------------
def ord32(x):
    """place_device.hpp, ord_f32: the unsigned that sorts like the float."""
    u = np.asarray(x, dtype=F32).view(np.uint32).astype(np.int64)
    return np.where(u >> 31, u ^ 0xffffffff, u ^ 0x80000000)


def unord32(o):
    o = np.asarray(o, dtype=np.int64)
    u = np.where(o >> 31, o ^ 0x80000000, o ^ 0xffffffff)
    return u.astype(np.uint32).view(F32)


def step(x, n):
    """x moved by n units in the last place (n > 0: towards +inf)."""
    return unord32(ord32(x) + int(n))[()]


# ---- scenes and their database ------------------------------------------------------------------------------------------
class Scene:
    """lists: one list of (branch, posting score) per k-mer of the read, branches ascending.  keep: the keep_at_most the
    scene is named for.  expect: what the restatement and the oracle must show (see check_scene)."""

    def __init__(self, name, lists, keep, expect, seam):
        self.name, self.keep, self.expect, self.seam = name, int(keep), dict(expect), seam
        self.lists = [sorted((int(b), F32(s)) for b, s in lst) for lst in (lists if lists and isinstance(lists[0], list) else [lists])]
        self.read = None


def _word(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def _codes(read, k):
    return [int("".join(str("ACGT".index(c)) for c in read[i:i + k]), 4) for i in range(len(read) - k + 1)]


def scene_db(num_branches, k, scenes):
    """One k-mer code per list; a scene's read spells its codes.  Returns (db, reads); sets scene.read."""
    num_codes, used, lists = 4 ** k, set(), {}
    free = iter(range(num_codes))
    for sc in sorted(scenes, key=lambda s: -len(s.lists)):          # the reads of several k-mers choose first
        if len(sc.lists) == 1:
            code = next(c for c in free if c not in used)
            read = _word(code, k)
        else:
            read = next(r for r in (_word(c, k) + "CG"[:len(sc.lists) - 1] for c in range(num_codes - 1, 0, -7))
                        if len(set(_codes(r, k))) == len(sc.lists) and not set(_codes(r, k)) & used)
        sc.read = read
        for code, lst in zip(_codes(read, k), sc.lists):
            used.add(code)
            lists[code] = lst
    offsets = np.zeros(num_codes + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(lists.get(c, ())) for c in range(num_codes)])
    values = np.zeros(int(offsets[-1]), dtype=PKDB_VALUE)
    at = 0
    for c in range(num_codes):
        for b, s in lists.get(c, ()):
            assert 0 <= b < num_branches and np.isfinite(s) and s <= 0 and not (s == 0 and np.signbit(s)), (c, b, s)
            values[at] = (b, s)
            at += 1
        br = [b for b, _ in lists.get(c, ())]
        assert br == sorted(set(br))
    db = SynthDB(states="nucl", kmer_size=k, omega=1.5, num_branches=int(num_branches), offsets=offsets, values=values)
    return db, [sc.read for sc in scenes]


def corrected_rows(db, read):
    """(branches ascending, corrected float32 scores, counts, float32 numerators) of the rows a read touches: place.cpp:418-422
    in float32, the postings added in the read's order."""
    k, n = db.kmer_size, db.num_branches
    total, count = np.zeros(n, dtype=F32), np.zeros(n, dtype=np.int64)
    codes = _codes(read, k)
    for code in codes:
        v = db.values[int(db.offsets[code]):int(db.offsets[code + 1])]
        total[v["branch"]] = total[v["branch"]] + v["score"]
        count[v["branch"]] += 1
    rows = np.nonzero(count)[0]
    pre = total[rows] + (F32(len(codes)) - count[rows].astype(F32)) * F32(db.log_threshold)
    with np.errstate(under="ignore"):
        return rows, (pre / F32(k)).astype(F32), count[rows], pre.astype(F32)


# ---- the selection's bookkeeping, restated ------------------------------------------------------------------------------
def dense_lanes(local_rows):
    return (np.asarray(local_rows) % 256) // 4


def listed_quads(quads, count_bytes):
    """The touched quads in the order list_touched_quads lists them: it reads 16 bytes of counts a lane (4 quads of 8-bit
    counts, 2 of 16-bit ones) and lists trip by trip, quad by quad of the 16 bytes, lane by lane."""
    per = 4 if count_bytes == 1 else 2
    quads = np.unique(np.asarray(quads))
    vec, j = quads // per, quads % per
    return quads[np.lexsort((vec % 64, j, vec // 64))]


def sparse_lanes(local_rows, count_bytes):
    """Lane of each row in the touched-quad epilogue, and the number of touched quads: entry i of the list belongs to lane i % 64."""
    listed = listed_quads(np.asarray(local_rows) // 4, count_bytes)
    position = {int(q): i for i, q in enumerate(listed)}
    return np.asarray([position[int(r) // 4] % 64 for r in local_rows], dtype=np.int64), len(listed)


def tau_search(lane_best, n_sel):
    """place_epilogue_body / tau_of_lane_maxima, line by line.  Returns (tau, the shortcut taken: 20, 24 or None)."""
    reached = lambda trial: int((lane_best >= trial).sum()) >= n_sel
    top, prefix, bit, shortcut = int(lane_best.max()), 0, 31, None
    for shared in (20, 24):
        trial = top & ~((1 << shared) - 1)
        if bit == 31 and trial != 0 and reached(trial):
            prefix, bit, shortcut = trial, shared - 1, shared
    if ((bit - TAU_STOP + 1) & 1) and bit >= TAU_STOP:
        if reached(prefix | (1 << bit)):
            prefix |= 1 << bit
        bit -= 1
    while bit > TAU_STOP:
        t1, t2, t3 = prefix | (1 << (bit - 1)), prefix | (2 << (bit - 1)), prefix | (3 << (bit - 1))
        prefix = t3 if reached(t3) else t2 if reached(t2) else t1 if reached(t1) else prefix
        bit -= 2
    return (prefix if prefix else 1), shortcut


def select_model(lanes, scores, keep, cap):
    """touched, n_sel, tau, n_cand and the ranking's path for the edges `scores` (float32) owned by `lanes`."""
    touched = len(scores)
    if touched == 0:
        return {"touched": 0, "n_sel": 0, "tau": 1, "n_cand": 0, "path": "none", "shortcut": None, "edge_lanes": 0, "kept_on_tau": False}
    o = ord32(scores)
    lane_best = np.zeros(64, dtype=np.int64)
    np.maximum.at(lane_best, lanes, o)
    n_sel = min(keep, touched)
    edge_lanes = int((lane_best != 0).sum())
    tau, shortcut = tau_search(lane_best, n_sel)
    rule = 1 if edge_lanes < n_sel else int(np.sort(lane_best)[::-1][n_sel - 1]) & ~255
    assert tau == rule, (tau, rule)            # the closed form of the issue, against the replayed search
    n_cand = touched if tau <= 1 else int((o >= tau).sum())
    assert n_cand >= n_sel
    rank_of_tau = int((o > tau).sum()) if (o == tau).any() else None      # a row exactly on tau, and how many rows beat it
    if cap == WAVE_CAP:
        path = "readlane" if n_cand <= 64 else "broadcast2" if n_cand <= 128 else "broadcast3" if n_cand <= 192 else "repeated"
    else:
        path = "readlane" if n_cand <= cap else "repeated"
    return {"touched": touched, "n_sel": n_sel, "tau": tau, "n_cand": n_cand, "path": path, "shortcut": shortcut,
            "edge_lanes": edge_lanes, "kept_on_tau": rank_of_tau is not None and rank_of_tau < n_sel}


def slice_models(rows, scores, keep, slices, slice_rows, count_bytes=None):
    """Per slice of a team layout (slice s: branches s R .. s R + R - 1, as partial_info() reports R): the model of its
    epilogue -- dense, or over the touched quads when count_bytes is given -- and its number of touched quads."""
    out = []
    for s in range(slices):
        mine = (rows // slice_rows) == s
        local = rows[mine] - s * slice_rows
        if count_bytes is None or not mine.any():
            lanes, quads = dense_lanes(local), len(np.unique(local // 4))
        else:
            lanes, quads = sparse_lanes(local, count_bytes)
        m = select_model(lanes, scores[mine], keep, SLICE_CAP)
        m["quads"] = quads
        out.append(m)
    return out


def merge_form(slices, keep, packed=True):
    m = slices * keep
    return "packed16" if packed and m <= 16 else "packed32" if packed and m <= 32 else "lanes" if m <= 64 else "loop"


def ranked(rows, scores, counts):
    """(score desc, branch asc), as the 64-bit key ord(score) << 32 | ~branch orders them."""
    order = np.lexsort((rows, -ord32(scores)))
    return rows[order], scores[order], counts[order]


def tie_group(scores_ranked, rank):
    """First and last rank of the rows that tie with the row of `rank`."""
    same = np.nonzero(scores_ranked.view(np.uint32) == scores_ranked[rank].view(np.uint32))[0]
    return int(same[0]), int(same[-1])


# ---- the scene groups -----------------------------------------------------------------------------------------------------
def _free_rows(span, used, first=()):
    """Rows of [0, span) not in `used`: where the kernel looks first (lane 0, lane 63, row 256, the last row, the partial last
    trip), then the rest."""
    last_trip = range((span - 1) // 256 * 256, span)
    prefer = list(first) + [0, 1, 2, 3, 252, 253, 254, 255, 256, span - 1, span - 2] + list(last_trip)
    seen, out = set(used), []
    for r in prefer + list(range(span)):
        if 0 <= r < span and r not in seen:
            seen.add(r)
            out.append(r)
    return out


def one_lane_scene(name, span, keep, n_cand, base=0, lane=5):
    """Group 1.  The best rows in the rows of ONE lane in successive trips, n_sel - 1 other lanes with one row each,
    descending; v, the lowest of those lane maxima, has ord & 255 == 255, so tau = ord(v) - 255, and fillers at
    ord(v) - 1, - 2, ... bring n_cand to the number asked for -- the last of them exactly ON tau, and one row more a unit
    BELOW tau, which is no candidate."""
    mine = [r for t in range((span + 255) // 256) for r in range(256 * t + 4 * lane, 256 * t + 4 * lane + 4) if r < span]
    n_best = min(keep, len(mine))
    others = [l for l in range(min(64, (span + 3) // 4)) if l != lane]
    n_other = min(keep, n_best + len(others)) - 1 if keep > 1 else 0
    pick = [others[i] for i in np.linspace(0, len(others) - 1, n_other).round().astype(int)] if n_other else []
    assert len(set(pick)) == n_other
    rows = {r: F32(-1.0 - 0.125 * i) for i, r in enumerate(mine[:n_best])}
    maxima = [F32(-5.0 - 0.25 * j) for j in range(n_other)] if n_other else []
    for l, s in zip(pick, maxima):
        rows[min(4 * l + l % 4, span - 1) if 4 * l + l % 4 < span else 4 * l] = s
    low_row = max(rows, key=lambda r: -rows[r])                      # the row that holds v
    v = unord32(ord32(rows[low_row]) | 255)[()]
    rows[low_row] = v
    n_fill = n_cand - len(rows)
    assert 0 <= n_fill <= 254, (name, n_fill)
    free = _free_rows(span, rows)
    for i in range(n_fill):
        rows[free[i]] = step(v, -255) if i == n_fill - 1 else step(v, -1 - i)
    rows[free[n_fill]] = step(v, -256)                               # a unit below tau
    expect = {"n_cand": n_cand, "best_lanes": 1}
    return Scene(name, [(base + r, F32(4.0) * s) for r, s in rows.items()], keep, expect,
                 f"best {n_best} rows in lane {lane}, n_cand = {n_cand}")


def wave_scenes():
    n, sc = WAVE_N, []
    # -- 1: top rows in one lane, the candidate counts on both sides of every path
    for n_cand in (1, 2, 3):
        sc.append(one_lane_scene(f"lane-keep1-cand{n_cand}", n, 1, n_cand))
    sc.append(one_lane_scene("lane-keep2-cand3", n, 2, 3))
    for n_cand in (63, 64, 65, 127, 128, 129, 191, 192, 193):
        sc.append(one_lane_scene(f"lane-keep7-cand{n_cand}", n, 7, n_cand, lane=(5, 0, 63)[n_cand % 3] if n_cand % 3 != 2 else 31))
    # -- 2: ties
    top6 = [(40 * i + 17, F32(-4.0 - i)) for i in range(6)]          # ranks 0 .. 5, distinct, one lane each
    for g, tied in ((2, (255, 512)), (3, (252, 300, 599)), (70, tuple(range(130, 130 + 6 * 70, 6)))):
        lower = [(r, F32(-80.0 - r)) for r in (1, 258, 598)]
        sc.append(Scene(f"tie{g}-straddles-keep", top6 + [(r, F32(-44.0)) for r in tied] + lower, 7,
                        {"tie_ranks": (6, 5 + g), "n_cand": 6 + g}, f"{g} rows tied over ranks 6 .. {5 + g}; the kept one is branch {tied[0]}"))
    sc.append(Scene("tie-all-lane-maxima", [(4 * l + (l % 4) + 256 * (l % 2), F32(-8.0)) for l in range(64)] +
                    [(4 * l + ((l + 1) % 4) + 256 * (l % 2), F32(-100.0 - l)) for l in range(64)], 7,
                    {"tie_ranks": (0, 63), "n_cand": 64, "path": "readlane"}, "all 64 lane maxima tied"))
    sc.append(Scene("tie-at-tau-over-cap", top6 + [(r, F32(-44.0)) for r in range(300, 500)], 7,
                    {"tie_ranks": (6, 205), "n_cand": 206, "path": "repeated"}, "200 rows tied at tau, six distinct rows above"))
    sc.append(Scene("tie-with-best-4-of-5", [(r, F32(-6.0)) for r in (9, 263, 530, 599)] + [(3, F32(-6.5))], 7,
                    {"top_tie": (0, 3), "n_cand": 5, "kept_at_factor_1": 4}, "four rows tie with the best: factor 1.0 keeps them"))
    on_tau = unord32(int(ord32(F32(-2.75))) & ~255)[()]               # ord & 255 == 0: v itself is tau
    sc.append(Scene("kept-row-on-tau", top6 + [(300, F32(4.0) * on_tau), (303, F32(-60.0))], 7, {"n_cand": 7, "kept_on_tau": True},
                    "the row of rank 6 has ord & 255 == 0: it lies exactly on tau, and `>` for `>=` would lose it"))
    # -- 3: near ties.  o0: bits 0 .. 24 of ord all ones (-0.125 corrected), rows at o0 - i d, i = 0 .. 7, seven kept
    o0 = (int(ord32(F32(-1.0))) & ~((1 << 25) - 1)) | ((1 << 25) - 1)
    spots = (599, 3, 264, 255, 530, 130, 140, 301)                  # eight lanes; the better rows are not the lower branches
    for d, shortcut, n_cand in ((1, 20, 8), (256, 20, 7), (512, 20, 7), (1 << 19, 24, 7), (1 << 20, 24, 7), (1 << 23, None, 7),
                                (1 << 24, None, 7)):
        rows = [(spots[i], F32(4.0) * unord32(o0 - i * d)[()]) for i in range(8)]
        sc.append(Scene(f"near-d{d}", rows, 7, {"n_cand": n_cand, "shortcut": shortcut, "ord_step": d},
                        f"eight rows {d} units apart, rank 6 | 7 among them; shortcut {shortcut}"))
    binade = [F32(-0.5), step(F32(-0.5), -1), step(F32(-1.0), 1), F32(-1.0), step(F32(-1.0), -1), step(F32(-2.0), 1), F32(-2.0),
              step(F32(-2.0), -1)]
    sc.append(Scene("near-binades", [(spots[i], F32(4.0) * s) for i, s in enumerate(binade)], 7,
                    {"tie_ranks": (6, 6), "binades": 3}, "pairs a unit apart on either side of -0.5, -1.0 and -2.0"))
    sc.append(Scene("near-far-from-top", [(77, F32(-4.0))] + [(spots[i], F32(4.0) * step(F32(-3000.0), -i)) for i in range(8)], 7,
                    {"shortcut": None, "n_cand": 9}, "one row at -1, eight a unit apart near -3000: neither shortcut"))
    # -- 4: touched against keep
    sc.append(Scene("touched0-absent", [], 7, {"touched": 0}, "the k-mer has no list"))
    for keep in KEEPS:
        for touched in sorted({1, keep - 1, keep, keep + 1} - {0}):
            rows = [((i * 37 + 255) % n, F32(-4.0 - 0.375 * ((i * 7) % touched))) for i in range(touched)]
            sc.append(Scene(f"touched{touched}-keep{keep}", rows, keep, {"touched": touched, "n_sel": min(keep, touched)},
                            f"touched = {touched} against keep = {keep}"))
    return sc


def second_wave_scenes():
    """The scenes kept away from keep_factor 1.0 (group 5: their like-weight ratios equal the best row's in double) and the
    reads of two and three k-mers."""
    n, sc = WAVE_N, []
    tiny = {10: F32(0.0), 11: F32(-2.0 ** -110), 9: F32(-5.0), 8: F32(-9.0),           # one quad: zero, tiny, ordinary
            300: F32(-2.0 ** -120), 301: F32(-12.0), 597: F32(-np.finfo(F32).tiny), 520: F32(-16.0), 140: F32(-20.0)}
    sc.append(Scene("zero-and-tiny", list(tiny.items()), 7, {"redo_trips": {0, 1, 2}, "first": (10, 597, 300, 11)},
                    "numerators 0.0, -2^-110, -2^-120, -2^-126 beside ordinary rows: every trip redoes its division"))
    sc.append(Scene("zero-alone-in-trip0", [(10, F32(0.0)), (9, F32(-4.0)), (301, F32(-12.0)), (597, F32(-3.0))], 2,
                    {"redo_trips": {0}, "first": (10, 597)}, "0.0 in trip 0 only"))
    # two lists that overlap in part: rows in one list only pick up log_thr; 20 (list A) and 21 (list B) tie exactly
    a = [(20, F32(-3.0)), (22, F32(-1.0)), (256, F32(-2.0)), (599, F32(-2.5))]
    b = [(21, F32(-3.0)), (22, F32(-1.5)), (256, F32(-0.5)), (300, F32(-7.0))]
    sc.append(Scene("two-kmers-overlap", [a, b], 2, {"tie_pair": (20, 21), "counts": {1, 2}},
                    "rows of count 1 and 2; branches 20 and 21 tie through different lists"))
    c = [(22, F32(-0.25)), (23, F32(-3.0)), (599, F32(-1.0))]
    sc.append(Scene("three-kmers-overlap", [a, b, c], 7, {"tie_pair": (20, 21), "counts": {1, 2, 3}}, "counts 1, 2 and 3"))
    # tau = 1 with more than 192 touched rows of distinct scores and mixed counts: 50 lanes hold an edge, keep = 64
    la = [(r, F32(-1.0 - 0.0101 * ((r * 31) % 211))) for r in range(0, 200)]
    lb = [(r, F32(-2.0 - 0.01307 * ((r * 17) % 151))) for r in list(range(100, 200)) + list(range(256, 306))]
    sc.append(Scene("slow-path-distinct", [la, lb], 64, {"tau": 1, "touched": 250, "path": "repeated", "counts": {1, 2}, "distinct": True},
                    "250 touched rows in 50 lanes, keep = 64: tau = 1, repeated selection over distinct keys"))
    return sc


def run_scenes():
    """Every list one ascending run of branches: a run-coded image stores such a list without its cells, and the kernels with
    the run path count per list (db_image.cpp, is_run)."""
    n = WAVE_N
    tied = [(r, F32(-44.0)) for r in range(300, 500)]
    ramp = [(r, F32(-4.0 - 0.03 * ((r * 7) % 300))) for r in range(300)]
    tail = [(r, F32(-4.0 - 0.5 * (r - 530)) if r < 536 else F32(-44.0)) for r in range(530, n)]
    quad = [(r, F32(-6.0 - 0.25 * (r % 4))) for r in range(252, 260)]
    return [Scene("run-200-tied", tied, 7, {"tie_ranks": (0, 199), "n_cand": 200, "path": "repeated"}, "a run of 200 tied rows"),
            Scene("run-300-distinct", ramp, 64, {"touched": 300, "distinct": True}, "a run over rows 0 .. 299, distinct scores"),
            Scene("run-to-the-last-row", tail, 7, {"tie_ranks": (6, 69), "n_cand": 70, "path": "broadcast2"},
                  "a run that ends on N - 1: six distinct rows, then 64 tied into the partial trip"),
            Scene("run-over-a-trip-seam", quad, 2, {"tie_ranks": (0, 1), "first": (252, 256)}, "rows 252 .. 259: a tie between lane 63 and lane 0 of the next trip"),
            Scene("run-of-one", [(n - 1, F32(-4.0))], 7, {"touched": 1}, "the last row alone")]


def all_runs(db):
    """Every list of the database is one ascending run (or empty)."""
    off = db.offsets.astype(np.int64)
    return all((np.diff(db.values["branch"][a:b].astype(np.int64)) == 1).all() for a, b in zip(off[:-1], off[1:]))


def stale_scenes():
    """What one read's candidate list leaves behind for the next read of the same wave.  The broadcast ranking reads four
    entries a trip, so with n_cand no multiple of 4 it reads up to three entries past the list, and must take them for
    nothing.  A "high" read leaves 192 candidates at -0.25 in the list; a "low" read behind it has 65, 66, 67, 129, 130 or 131
    candidates, all below -4: an entry of the high read that counted would outrank every row of the low one.  The reads
    alternate irregularly, so that a wave meets a low read behind a high one however the grid deals the reads out."""
    sc, lows = [], (65, 66, 67, 129, 130, 131)
    for i in range(40):
        if (i * i + i // 3) % 5 in (0, 1):
            rows = [(200 + r, F32(-1.0)) for r in range(192)]
            sc.append(Scene(f"stale-high-{i}", rows, 7, {"n_cand": 192, "path": "broadcast3"}, "192 candidates at -0.25"))
        else:
            n_cand = lows[i % len(lows)]
            rows = [(40 * j + 17 + i % 3, F32(-16.0 - 0.5 * j)) for j in range(6)] + [(300 + r, F32(-20.0)) for r in range(n_cand - 6)]
            sc.append(Scene(f"stale-low-{i}", rows, 7, {"n_cand": n_cand, "path": "broadcast2" if n_cand <= 128 else "broadcast3",
                                                       "tie_ranks": (6, n_cand - 1)}, f"{n_cand} candidates below -4: {-n_cand % 4} spare entries read"))
    assert {len(x.lists[0]) for x in sc} == {192} | set(lows)
    return sc


def fast_division_differs(numerator, k):
    """Whether the three-instruction division by k (place_device.hpp, div_k: y = RN(1 / k); q = RN(x y); r = fma(-q, k, x);
    fma(r, y, q)) misses the IEEE quotient of a DENORMAL float32 numerator: there every value is a whole number of units
    u = 2^-149, RN is Python's round (ties to even) on exact fractions, and r is exact."""
    from fractions import Fraction
    x = Fraction(float(numerator)) / Fraction(2) ** -149
    assert x.denominator == 1 and abs(x) < 2 ** 23
    y = Fraction(float(F32(1.0) / F32(k)))
    q = round(x * y)
    return round(q + (x - q * k) * y) != round(x / k)


def division_scenes(base=0):
    """k = 6: the numerators -21 u and -33 u (u = 2^-149) have the quotients -3.5 u and -5.5 u, ties that IEEE division
    rounds to -4 u and -6 u and the three-instruction division to -3 u and -5 u; -15 u and -27 u come out alike.  The kernels
    redo a trip that meets |x| < 2^-100 with the exact division; with k = 4 and 5 no float32 numerator needs it."""
    u = 2.0 ** -149
    rows = [(base + 8, F32(-33 * u)), (base + 9, F32(-27 * u)), (base + 10, F32(-21 * u)), (base + 11, F32(-15 * u)),
            (base + 40, F32(-6.0)), (base + 41, F32(-9.0))]
    return [Scene("tiny-ties-of-the-division", rows, 7, {"fast_division_differs": {base + 8, base + 10}, "first": (base + 11, base + 9, base + 10, base + 8)},
                  "quotients -2.5 u, -4.5 u, -3.5 u, -5.5 u: the last two only by the redone division")]


def small_scenes():
    """A tree of three branches: fewer than keep."""
    return [Scene("n3-touched0", [], 7, {"touched": 0}, "no list, N = 3 < keep"),
            Scene("n3-touched1", [(2, F32(-4.0))], 7, {"touched": 1}, "the last branch alone"),
            Scene("n3-touched3", [(0, F32(-4.0)), (1, F32(-4.0)), (2, F32(-2.0))], 2, {"touched": 3, "tie_ranks": (1, 2)},
                  "branches 0 and 1 tie over rank 1 | 2")]


def edge_n_scenes(n):
    """N = 63 (the dummy row right behind the last branch) and 256 (one whole trip, the dummy row in a block of its own)."""
    sc = [one_lane_scene(f"n{n}-lane-cand{c}", n, 1, c, lane=(n - 1) // 4 % 64 if n < 256 else 63) for c in (1, min(n, 65) - 2)]
    sc.append(Scene(f"n{n}-tie-first-last", [(0, F32(-4.0)), (n - 1, F32(-4.0)), (n // 2, F32(-4.0)), (1, F32(-9.0))], 2,
                    {"tie_ranks": (0, 2)}, "rows 0, N / 2 and N - 1 tie over rank 1 | 2"))
    sc.append(Scene(f"n{n}-all-rows", [(r, F32(-1.0 - 0.3 * ((r * 29) % n))) for r in range(n)], 64, {"touched": n},
                    "every branch touched, distinct scores"))
    return sc


def team_scenes(n, slices):
    """Group 7, for slices of R = ceil(N / slices) rows."""
    r_, sc = -(-n // slices), []
    first, last = lambda s: s * r_, lambda s: min(n, (s + 1) * r_) - 1
    keep = 4
    rows = [(first(1) + i, F32(-4.0 - 0.75 * i)) for i in range(min(r_, 9))]
    sc.append(Scene("team-all-in-slice1", rows, keep, {"kept_slices": {1}, "touched_slices": {1}}, "every kept row in slice 1, the others untouched"))
    rows = [(last(s) if s % 2 else first(s), F32(-4.0 - ((s * 3) % slices))) for s in range(slices)]
    sc.append(Scene("team-one-row-a-slice", rows, max(keep, slices), {"kept_slices": set(range(slices))}, "one kept row a slice"))
    rows = [(last(0), F32(-4.0)), (first(1), F32(-4.0)), (first(0), F32(-6.0)), (first(1) + 2, F32(-6.0)), (last(slices - 1), F32(-6.0))]
    sc.append(Scene("team-tie-over-a-seam", rows, 4, {"tie_ranks": (2, 4), "pair_top": (last(0), first(1))},
                    "last row of slice 0 ties with the first of slice 1; three more tie over rank 3 | 4"))
    rows = [((first(s) + last(s)) // 2, F32(-4.0)) for s in range(slices)] + [(first(s) + 1, F32(-7.0 - s)) for s in range(slices)]
    sc.append(Scene("team-tie-across-slices", rows, 4, {"top_tie": (0, slices - 1)}, "one row of every slice in one tie"))
    rows = [(first(0) + 1, F32(-5.0)), (first(0) + 2, F32(-4.5))] + [(first(1) + i, F32(-4.0 - 0.25 * ((i * 5) % min(r_, 12)))) for i in range(min(r_, 12))]
    sc.append(Scene("team-few-beside-many", rows, 4, {"slice_touched": {0: 2, 1: min(r_, 12)}}, "a slice with touched < keep beside one with more"))
    on_tau = unord32(int(ord32(F32(-2.75))) & ~255)[()]
    rows = [(first(1) + 4 * j, F32(-4.0 - j)) for j in range(3)] + [(first(1) + 12, F32(4.0) * on_tau), (first(1) + 13, F32(-60.0)),
                                                                     (last(0), F32(0.0))]
    sc.append(Scene("team-kept-row-on-tau", rows, 4, {"slice_kept_on_tau": {0: True, 1: True}, "pair_top": (last(0), first(1))},
                    "slice 0 holds one row, 0.0, its own tau; in slice 1 the fourth of four lane maxima has ord & 255 == 0"))
    if r_ >= 65:
        for n_cand in (59, 60, 61):
            s = one_lane_scene(f"team-slice1-cand{n_cand}", min(r_, last(1) - first(1) + 1), keep, n_cand, base=first(1), lane=3)
            s.lists[0] += [(first(0) + 5, F32(-9.0)), (first(0) + 6, F32(-9.5))]     # slice 0 beside it: two rows, the fast path
            s.lists[0].sort()
            s.expect = {"slice_n_cand": {0: 2, 1: n_cand}, "slice_path": {0: "readlane", 1: "readlane" if n_cand <= 60 else "repeated"}}
            sc.append(s)
        rows = [(first(0) + i, F32(-3.0 - 0.125 * ((i * 11) % 64))) for i in range(64)] + [(first(1) + i, F32(-3.03 - i)) for i in range(5)]
        sc.append(Scene("team-keep64-slow-slice", rows, 64, {"slice_touched": {0: 64, 1: 5}, "slice_path": {0: "repeated", 1: "readlane"}},
                        "keep = 64: a slice with 64 touched rows selects repeatedly, its neighbour does not"))
    return sc


def quad_scenes():
    """The touched-quad epilogue: lists that touch row 4 i of slice 0 for i below the count, the best rows in the first and the
    last listed quad; slice 1 holds two rows."""
    r_, sc = QUAD_N // 2, []
    for q in QUAD_COUNTS:
        rows = {4 * i: F32(-8.0 - 0.001 * ((i * 131) % 257)) for i in range(q)}
        rows[0], rows[4 * (q - 1)] = F32(-2.0), (F32(-1.0) if q > 1 else F32(-2.0))
        for width, score in ((1, F32(-2.5)), (2, F32(-2.75))):        # ... and in the quad either count width lists last
            if 4 * int(listed_quads(np.arange(q), width)[-1]) not in (0, 4 * (q - 1)):
                rows[4 * int(listed_quads(np.arange(q), width)[-1])] = score
        rows[r_ + 3], rows[QUAD_N - 1] = F32(-1.5), F32(-30.0)
        sc.append(Scene(f"quads{q}", list(rows.items()), 7, {"slice_quads": {0: q, 1: 2}, "ends_kept": True, "top3": tuple(sorted({4 * (q - 1), r_ + 3, 0}, key=lambda r: -rows[r]))},
                        f"{q} touched quads in slice 0"))
    return sc


# ---- the databases the GPU file places -----------------------------------------------------------------------------------
_CACHE = {}


def database(name, k):
    """(db, reads, packed reads, scenes, N, slices or None) of a database, built once."""
    key = ("db", name, k)
    if key not in _CACHE:
        slices = None
        if name == "wave":
            n, scenes = WAVE_N, wave_scenes()
        elif name == "wave2":
            n, scenes = WAVE_N, second_wave_scenes()
        elif name == "runs":
            n, scenes = WAVE_N, run_scenes()
        elif name == "stale":
            n, scenes = WAVE_N, stale_scenes()
        elif name == "div6":
            n, scenes = WAVE_N, division_scenes()
        elif name == "div6team":
            n, slices, scenes = TEAM_N[4], 4, division_scenes(base=TEAM_N[4] // 4)
        elif name == "n3":
            n, scenes = 3, small_scenes()
        elif name in ("n63", "n256"):
            n, scenes = int(name[1:]), edge_n_scenes(int(name[1:]))
        elif name == "quads":
            n, slices, scenes = QUAD_N, 2, quad_scenes()
        else:
            slices = int(name[len("team"):])
            n, scenes = TEAM_N[slices], team_scenes(TEAM_N[slices], slices)
        db, reads = scene_db(n, k, scenes)
        _CACHE[key] = (db, reads, pack_reads(reads), scenes, n, slices)
    return _CACHE[key]


KS = {"div6": (6,), "div6team": (6,)}         # k of a database: 4 (exact quotients) and 5 unless named here


def ks_of(name):
    return KS.get(name, (4, 5))


DATABASES = ("wave", "wave2", "runs", "stale", "div6", "div6team", "n3", "n63", "n256", "team2", "team4", "team8", "quads")


def settings(name):
    """(keep_at_most, keep_factor) of every placement of a database in the GPU file: every keep its scenes are named for at the
    usual factor, and keep = 7 at the other factors where the filter is the subject.  The zero and tiny sums of "wave2" stay
    away from factor 1.0, and the tiny quotients of "div6" from every factor but 0: their ratios equal the best row's."""
    if name.startswith("div6"):
        return [(7, 0.0), (2, 0.0)]
    few = {"runs": (2, 7, 64), "stale": (7,), "n256": (1, 2, 64), "n63": (1, 2, 64), "n3": (2, 7)}
    if name in few:
        assert {sc.keep for sc in database(name, 4)[3]} <= set(few[name])
        return [(keep, 0.01) for keep in few[name]]
    slices = database(name, 4)[5]
    keeps = KEEPS if slices is None else tuple(sorted(set(TEAM_KEEPS[slices]) | {7}))
    return [(keep, 0.01) for keep in keeps] + [(7, f) for f in FACTORS if f != 0.01 and not (name == "wave2" and f == 1.0)]


def reference(oracle_lib, name, k, keep, factor):
    """The oracle's (rows, n_rows, counts) of a database's reads, computed once and shared; read-only."""
    key = ("ref", name, k, int(keep), float(factor))
    if key not in _CACHE:
        db, _, (data, offs), *_ = database(name, k)
        out = oracle_lib.Oracle.from_synth(db, keep_at_most=keep, keep_factor=factor).place(data, offs, num_threads=0)
        for a in out:
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


# ---- per scene: the restatement against the oracle, and the seam the scene is named for ---------------------------------
def check_scene(oracle_lib, name, k, index, sc, named):
    """Returns the line that lists the scene.  named: assert sc.expect (the first k of the database); else only restatement == oracle."""
    db, reads, _, _, n, slices = database(name, k)
    keep, e = sc.keep, sc.expect
    rows, scores, counts, pre = corrected_rows(db, sc.read)
    ref_rows, ref_n, ref_counts = reference(oracle_lib, name, k, keep, 0.0)
    want_b, want_s, want_c = ranked(rows, scores, counts)
    n_sel = min(keep, len(rows))
    if len(rows):       # the restated corrected scores and their order ARE the oracle's
        assert int(ref_n[index]) == n_sel, (sc.name, ref_n[index], n_sel)
        assert np.array_equal(ref_rows[index]["branch"][:n_sel], want_b[:n_sel]), sc.name
        assert np.array_equal(ref_rows[index]["score"][:n_sel].view(np.uint32), want_s[:n_sel].view(np.uint32)), sc.name
        assert np.array_equal(ref_counts[index][:n_sel], want_c[:n_sel]), sc.name
    else:               # :141-152: the first keep branches at the threshold score, count 0
        assert int(ref_n[index]) == keep and list(ref_rows[index]["branch"]) == list(range(keep)) and not ref_counts[index].any()
    wave = select_model(dense_lanes(rows), scores, keep, WAVE_CAP)
    got = {"touched": wave["touched"], "n_sel": wave["n_sel"], "tau": wave["tau"], "n_cand": wave["n_cand"], "path": wave["path"],
           "shortcut": wave["shortcut"], "kept_on_tau": wave["kept_on_tau"]}
    if len(rows):
        got["tie_ranks"] = tie_group(want_s, min(keep, len(rows)) - 1)
        got["top_tie"] = tie_group(want_s, 0)
        got["best_lanes"] = len(set(dense_lanes(want_b[:n_sel]).tolist()))
        got["ord_step"] = int(np.diff(np.sort(ord32(scores))).min()) if len(rows) > 1 else 0
        got["binades"] = len(set((np.frexp(scores[:])[1]).tolist()))
        got["redo_trips"] = set((rows[np.abs(pre) < F32(2.0 ** -100)] // 256).tolist())
        got["first"] = tuple(int(b) for b in want_b[:len(e.get("first", ()))])
        got["counts"] = set(counts.tolist())
        got["fast_division_differs"] = {int(b) for b, x in zip(rows, pre) if x != 0 and abs(x) < F32(2.0 ** -127)
                                        and fast_division_differs(x, k)}
        got["distinct"] = len(set(ord32(scores).tolist())) == len(rows)
        got["top3"] = tuple(int(b) for b in want_b[:len(e.get("top3", ()))])
        if "tie_pair" in e:
            i, j = (int(np.nonzero(rows == b)[0][0]) for b in e["tie_pair"])
            got["tie_pair"] = e["tie_pair"] if scores[i].view(np.uint32) == scores[j].view(np.uint32) else None
        if "pair_top" in e:
            got["pair_top"] = tuple(int(b) for b in want_b[:2])
        if "kept_at_factor_1" in e:
            got["kept_at_factor_1"] = int(reference(oracle_lib, name, k, keep, 1.0)[1][index])
    line = f"{name} k={k} {sc.name}: keep {keep}, touched {wave['touched']}, n_cand {wave['n_cand']} ({wave['path']}), tau {wave['tau']:#x}"
    if slices:
        r_ = -(-n // slices)
        dense = slice_models(rows, scores, keep, slices, r_)
        got["slice_touched"] = {s: m["touched"] for s, m in enumerate(dense) if s in e.get("slice_touched", ())}
        got["slice_n_cand"] = {s: m["n_cand"] for s, m in enumerate(dense) if s in e.get("slice_n_cand", ())}
        got["slice_path"] = {s: m["path"] for s, m in enumerate(dense) if s in e.get("slice_path", ())}
        got["slice_kept_on_tau"] = {s: m["kept_on_tau"] for s, m in enumerate(dense) if s in e.get("slice_kept_on_tau", ())}
        got["slice_quads"] = {s: m["quads"] for s, m in enumerate(dense) if s in e.get("slice_quads", ())}
        got["touched_slices"] = {s for s, m in enumerate(dense) if m["touched"]}
        got["kept_slices"] = set((want_b[:n_sel] // r_).tolist())
        line = (f"{name} k={k} {sc.name}: keep {keep}, merge {merge_form(slices, keep)}, per slice (touched, quads, n_cand, path) "
                f"{[(m['touched'], m['quads'], m['n_cand'], m['path']) for m in dense]}")
        got["ends_kept"] = True
        for width in (1, 2):    # the touched-quad epilogue owns rows by the list's order: other lanes, so another tau and n_cand
            sparse = slice_models(rows, scores, keep, slices, r_, count_bytes=width)
            assert [m["quads"] for m in sparse] == [m["quads"] for m in dense]
            if "slice_kept_on_tau" in e:
                assert {s: m["kept_on_tau"] for s, m in enumerate(sparse) if s in e["slice_kept_on_tau"]} == got["slice_kept_on_tau"]
            if "slice_n_cand" in e:
                assert {s: m["n_cand"] for s, m in enumerate(sparse) if s in e["slice_n_cand"]} == got["slice_n_cand"], (sc.name, width)
                assert {s: m["path"] for s, m in enumerate(sparse) if s in e["slice_path"]} == got["slice_path"], (sc.name, width)
            listed = listed_quads(rows[rows < r_] // 4, width)                    # slice 0: first and last listed quad hold a kept row
            if len(listed):
                got["ends_kept"] &= all(4 * int(q) in want_b[:n_sel] for q in (listed[0], listed[-1]))
            line += f"; quad epilogue, {8 * width}-bit counts: n_cand {[m['n_cand'] for m in sparse]}"
    if named:
        assert e, sc.name
        for what, want in e.items():
            assert got[what] == want, f"{name} {sc.name}: {what} is {got[what]}, the scene is named for {want}"
    return line + f" -- {sc.seam}"


@pytest.mark.parametrize("name,k", [(name, k) for name in DATABASES for k in ks_of(name)])
def test_every_scene_reaches_its_seam(oracle_lib, name, k):
    db, reads, _, scenes, n, slices = database(name, k)
    assert len(reads) <= 256 and len(set(reads)) == len(reads)
    for index, sc in enumerate(scenes):
        print(check_scene(oracle_lib, name, k, index, sc, named=(k == ks_of(name)[0])))


def test_the_scene_groups_cover_the_seams_of_the_issue(oracle_lib):
    """Across the k = 4 scenes: every candidate count on either side of a path, every path, every shortcut, every merge form."""
    seen, paths, shortcuts, slice_cands, slice_paths = set(), set(), set(), set(), set()
    assert all_runs(database("runs", 4)[0]) and all_runs(database("runs", 5)[0]) and not all_runs(database("wave", 4)[0])
    for name in ("wave", "wave2", "n63", "n256"):
        db, _, _, scenes, n, _ = database(name, 4)
        for sc in scenes:
            rows, scores, _, _ = corrected_rows(db, sc.read)
            m = select_model(dense_lanes(rows), scores, sc.keep, WAVE_CAP)
            seen.add(m["n_cand"]), paths.add(m["path"]), shortcuts.add(m["shortcut"])
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193} <= seen
    assert paths == {"none", "readlane", "broadcast2", "broadcast3", "repeated"} and shortcuts == {None, 20, 24}
    for name in ("team2", "team4"):
        db, _, _, scenes, n, slices = database(name, 4)
        for sc in scenes:
            rows, scores, _, _ = corrected_rows(db, sc.read)
            for m in slice_models(rows, scores, sc.keep, slices, -(-n // slices)):
                slice_cands.add(m["n_cand"]), slice_paths.add(m["path"])
    assert {59, 60, 61} <= slice_cands and slice_paths == {"none", "readlane", "repeated"}
    forms = {(merge_form(s, keep), s * keep) for s, keeps in TEAM_KEEPS.items() for keep in keeps}
    assert {m for _, m in forms} >= {16, 18, 20, 32, 36, 64, 66, 72}
    assert {f for f, _ in forms} == {"packed16", "packed32", "lanes", "loop"}
    assert merge_form(2, 8) == "packed16" and merge_form(2, 9) == "packed32" and merge_form(4, 8) == "packed32"
    assert merge_form(4, 9) == "lanes" and merge_form(8, 8) == "lanes" and merge_form(2, 33) == "loop"
    assert merge_form(2, 8, packed=False) == "lanes"


def test_the_ratio_filter_is_not_tested_on_its_rounding(oracle_lib):
    """No kept or dropped row's like-weight ratio lies within 1e-9 (relative) of best_ratio * keep_factor unless its score equals
    the best row's bit for bit: glibc's pow and the device's exp10 differ by units in the last place, and such a row would
    test them, not the filter."""
    checked = 0
    for name in DATABASES:
        for k in ks_of(name):
            for keep, factor in settings(name):
                full = reference(oracle_lib, name, k, keep, 0.0)
                got = reference(oracle_lib, name, k, keep, factor)
                for i in range(len(full[1])):
                    lwr, score = full[0][i]["lwr"][:full[1][i]], full[0][i]["score"][:full[1][i]]
                    thr = lwr[0] * factor
                    near = (np.abs(lwr - thr) <= 1e-9 * thr) & (thr > 0)   # (factor 0.0 keeps every row, 10^-512 == 0 included)
                    assert not (near & (score.view(np.uint32) != score[0].view(np.uint32))).any(), (name, k, keep, factor, i)
                    assert int(got[1][i]) == int((lwr >= thr).sum())
                    checked += 1
    assert checked > 1000


def test_steps_and_the_restated_key():
    assert step(F32(-1.0), 1) == np.nextafter(F32(-1.0), F32(0)) and step(F32(-1.0), -1) == np.nextafter(F32(-1.0), F32(-2))
    assert int(ord32(F32(0.0))) == 0x80000000 and int(ord32(F32(-1.0))) == 0x407fffff
    x = np.asarray([-3000.0, -2.0, -1.0, -0.5, -1e-39, 0.0], dtype=F32)
    assert (np.diff(ord32(x)) > 0).all() and np.array_equal(unord32(ord32(x)).view(np.uint32), x.view(np.uint32))
    # the touched-quad list: 8-bit counts put quads 0, 4, 8 ... first (quad j of every lane's 16 bytes), 16-bit ones 0, 2, 4 ...
    lanes, quads = sparse_lanes(np.arange(0, 40, 4), 1)
    assert quads == 10 and lanes.tolist() == [0, 3, 6, 8, 1, 4, 7, 9, 2, 5]
    lanes, quads = sparse_lanes(np.arange(0, 40, 4), 2)
    assert lanes.tolist() == [0, 5, 1, 6, 2, 7, 3, 8, 4, 9]
