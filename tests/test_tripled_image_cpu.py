"""The tripled k-mer table (db_layout.h: kTripled; epik_amd/csrc/db_image.cpp) without a device: every slot of every
block against a numpy restatement of its description, the posting region against the paired image's, and the rule that
chooses it (plan and plan_sizes)."""
import numpy as np
import pytest

from epik_amd import capi, placer as eplacer, synth

LINE = 128
ENTRY_BITS = 42
TRIPLED, PAIRED = 6, 3


def _bits(v):
    return int(v).bit_length()


def _entries(db, n_pad):
    """Per code: (len, first cell, line) of its run-coded list -- scores only, 4 bytes a posting, on whole lines, the
    lists in code order; an absent code (0, 0, 0)."""
    offs = db.offsets.astype(np.int64)
    lens = np.diff(offs)
    br = db.values["branch"].astype(np.int64)
    first = np.where(lens > 0, n_pad - 1 - br[np.minimum(offs[:-1], len(br) - 1)], 0)
    lines_of = (lens * 4 + LINE - 1) // LINE
    line = np.concatenate([[0], np.cumsum(lines_of)[:-1]])
    line = np.where(lens > 0, line, 0)
    for k in np.flatnonzero(lens > 1):  # (the restatement holds for run lists only: the test's databases are such)
        assert (np.diff(br[offs[k]:offs[k + 1]]) == 1).all()
    return lens, first, line, int(lines_of.sum())


def _decode(table, block, slot):
    """The 42 bits at bit 42 * slot of the 128-byte block."""
    word = int.from_bytes(table[block * LINE:(block + 1) * LINE].tobytes(), "little")
    return (word >> (ENTRY_BITS * slot)) & ((1 << ENTRY_BITS) - 1)


def _code_of(k, x, slot):
    """The code that belongs in `slot` of block x (a (k-1)-mer): a.X, X.b, or X[1:].b.b'."""
    blocks = 4 ** (k - 1)
    if slot < 4:
        return slot * blocks + x
    if slot < 8:
        return x * 4 + (slot - 4)
    return (x % 4 ** (k - 2)) * 16 + (slot - 8)


def _make(k):
    tree = synth.make_tree(60, seed=7)  # N = 119
    return synth.make_db(tree.num_nodes, kmer_size=k, seed=8, p_present=0.5, lognormal=(2.5, 1.5))


@pytest.fixture(scope="module", params=[5, 3])
def db(request):
    return _make(request.param)


@pytest.fixture()
def forced(monkeypatch):
    for var in ("EPIK_AMD_RUN_COUNTS", "EPIK_AMD_RING_FORM"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "tripled")
    return monkeypatch


def test_every_slot_of_every_block_and_the_postings(db, forced):
    k = db.kmer_size
    plan, table, filt, postings = eplacer.build_image(db)
    assert plan.layout == TRIPLED and plan.kernel == 0 and plan.run_coded == 1 and plan.filter_bytes == 0
    blocks = 4 ** (k - 1)
    assert plan.table_bytes == blocks * LINE + 8 and not table[blocks * LINE:].any()
    forced.setenv("EPIK_AMD_LAYOUT", "paired")
    p_plan, p_table, _, p_postings = eplacer.build_image(db)
    assert p_plan.layout == PAIRED and p_plan.table_bytes == 4 ** k * 16 + 8
    assert postings.tobytes() == p_postings.tobytes()

    n_pad = (db.num_branches + 1 + 63) // 64 * 64
    lens, first, line, n_lines = _entries(db, n_pad)
    assert plan.posting_bytes == n_lines * LINE + 512
    len_bits, cell_bits = _bits(db.num_branches), _bits(n_pad - 1)
    want = lens | (first << len_bits) | (line << (len_bits + cell_bits))
    assert int(want.max()) < 1 << ENTRY_BITS
    seen = np.zeros(4 ** k, dtype=np.int64)
    for x in range(blocks):
        word = int.from_bytes(table[x * LINE:(x + 1) * LINE].tobytes(), "little")
        assert word >> (ENTRY_BITS * 24) == 0, "the block's last 16 bits"
        for slot in range(24):
            code = _code_of(k, x, slot)
            assert (word >> (ENTRY_BITS * slot)) & ((1 << ENTRY_BITS) - 1) == int(want[code]), (x, slot, code)
            seen[code] += 1
    assert (seen == 6).all(), "every code is stored six times"
    # ... and against the paired table's own entries (len | first cell << 16, line)
    pairs = p_table[:-8].view(np.uint32).reshape(-1, 8, 2)
    for x in range(0, blocks, 7):
        for a in range(4):
            e = _decode(table, x, a)
            if pairs[x, a, 0] == 0:  # (the paired table gives an absent code the line of the next list; here it is all zero)
                assert e == 0
                continue
            assert [(e & ((1 << len_bits) - 1)) | (((e >> len_bits) & ((1 << cell_bits) - 1)) << 16),
                    e >> (len_bits + cell_bits)] == pairs[x, a].tolist()


def test_sparse_descriptor_builds_the_same_image(db, forced):
    dense = eplacer.build_image(db)
    sparse = eplacer.build_image(db, sparse=True)
    assert dense[0].layout == TRIPLED == sparse[0].layout
    for name in ("table_bytes", "filter_bytes", "posting_bytes", "kept_entries", "run_coded"):
        assert getattr(dense[0], name) == getattr(sparse[0], name), name
    for a, b in zip(dense[1:], sparse[1:]):
        assert a.tobytes() == b.tobytes()


def _fields(p):
    return {name: (list(getattr(p, name)) if name == "resident_waves" else getattr(p, name))
            for name, _ in capi.Plan._fields_ if name != "posting_bytes_is_bound"}


def test_plan_sizes_is_the_plan_with_the_layout_forced(db, forced):
    real = eplacer.plan(db)
    sized = eplacer.plan_sizes(states=db.states, kmer_size=db.kmer_size, num_branches=db.num_branches,
                               bins=eplacer.list_bins(db))
    assert real.layout == TRIPLED and _fields(sized) == _fields(real)


def _clear(monkeypatch):
    for var in ("EPIK_AMD_KERNEL", "EPIK_AMD_LAYOUT", "EPIK_AMD_RUNS", "EPIK_AMD_RUN_COUNTS", "EPIK_AMD_RING_FORM"):
        monkeypatch.delenv(var, raising=False)


# the headline's shape from a histogram alone: N = 999, k = 10, 60 % of the codes present, every list a run -- 500 000 of
# 59 postings (three lines with explicit cells, two run-coded) and 129 145 of 86 (five, three): 292 MB explicit, which
# run-coding brings inside the Infinity Cache (195 MB with the paired table of 16.8 MB, 211 MB with the tripled one)
HEADLINE = dict(states="nucl", kmer_size=10, num_branches=999)
HEADLINE_BINS = [(59, 500000, 500000), (86, 129145, 129145)]


def test_default_rule_takes_the_headline_shape(monkeypatch):
    _clear(monkeypatch)
    p = eplacer.plan_sizes(bins=HEADLINE_BINS, **HEADLINE)
    assert p.kernel == 0 and p.run_coded == 1 and p.layout == TRIPLED and p.table_bytes == 4 ** 9 * LINE + 8
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "tripled")
    assert _fields(eplacer.plan_sizes(bins=HEADLINE_BINS, **HEADLINE)) == _fields(p)
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "paired")
    q = eplacer.plan_sizes(bins=HEADLINE_BINS, **HEADLINE)
    assert q.layout == PAIRED and q.table_bytes == 4 ** 10 * 16 + 8 and q.posting_bytes == p.posting_bytes
    # what keeps the paired table: the run ring, the far form, a shard, a list that is no run
    for var, value in (("EPIK_AMD_RUN_COUNTS", "ring"), ("EPIK_AMD_RING_FORM", "far")):
        _clear(monkeypatch)
        monkeypatch.setenv(var, value)
        assert eplacer.plan_sizes(bins=HEADLINE_BINS, **HEADLINE).layout == PAIRED
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    assert eplacer.plan_sizes(bins=[(n, lists // 2, lists // 2) for n, lists, _ in HEADLINE_BINS], shard_index=0, shard_count=2,
                              **HEADLINE).layout == PAIRED
    assert eplacer.plan_sizes(bins=[(59, 500000, 499999), HEADLINE_BINS[1]], **HEADLINE).layout == PAIRED


def test_default_rule_keeps_the_image_inside_the_infinity_cache(monkeypatch):
    """Paired image 16.8 + 238 MB = inside 256 MiB, tripled 33.5 + 238 MB = beyond: paired stays."""
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    lists = (238 << 20) // 256
    assert lists <= 4 ** 10
    p = eplacer.plan_sizes(bins=[(59, lists, lists)], **HEADLINE)
    assert p.layout == PAIRED and p.table_bytes + p.posting_bytes <= 256 << 20 < 4 ** 9 * LINE + p.posting_bytes


def test_default_rule_leaves_small_tables_paired(db, monkeypatch):
    """k <= 8: the paired table is at most 1 MiB, inside one XCD's L2."""
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    assert eplacer.plan(db).layout == PAIRED
    sized = eplacer.plan_sizes(states="nucl", kmer_size=8, num_branches=999, bins=[(59, 30000, 30000)])
    assert sized.layout == PAIRED and sized.run_coded == 1
    real, sizes = eplacer.plan(db), eplacer.plan_sizes(states=db.states, kmer_size=db.kmer_size,
                                                       num_branches=db.num_branches, bins=eplacer.list_bins(db))
    assert _fields(real) == _fields(sizes)


def test_a_paired_table_of_exactly_4_mib_stays(monkeypatch):
    """k = 9: 4^9 entries of 16 bytes are exactly one XCD's L2, not larger: paired; k = 10 with the same lists: tripled."""
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    bins = [(59, 150000, 150000)]
    assert eplacer.plan_sizes(states="nucl", kmer_size=9, num_branches=999, bins=bins).layout == PAIRED
    assert eplacer.plan_sizes(states="nucl", kmer_size=10, num_branches=999, bins=bins).layout == TRIPLED


def test_entries_of_43_bits(monkeypatch):
    """N = 999 takes 10 + 10 bits, which leaves 22 for the line: 2^22 lists of two lines each are 2^23 lines."""
    _clear(monkeypatch)
    shape = dict(states="nucl", kmer_size=12, num_branches=999)
    bins = [(59, 1 << 22, 1 << 22)]
    assert eplacer.plan_sizes(bins=bins, **shape).layout == PAIRED
    assert eplacer.plan_sizes(bins=[(59, 1 << 20, 1 << 20)], **shape).layout == TRIPLED  # 2^21 lines: 42 bits
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "tripled")
    with pytest.raises(capi.EpikAmdError, match="42 bits"):
        eplacer.plan_sizes(bins=bins, **shape)


@pytest.mark.parametrize("num_branches", [1303, 1999])
def test_the_mid_size_trees_do_not_fit_at_k_10(num_branches, monkeypatch):
    """N = 1 303 and 1 999 take 11 + 11 bits for len and first cell; the headline's 1.5 M posting lines need 21 more: 43.
    Run-coded (EPIK_AMD_RUNS=1) they keep the paired table, and the tripled one is refused when forced."""
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    monkeypatch.setenv("EPIK_AMD_KERNEL", "wave")
    shape = dict(states="nucl", kmer_size=10, num_branches=num_branches)
    assert eplacer.plan_sizes(bins=HEADLINE_BINS, **shape).layout == PAIRED
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "tripled")
    with pytest.raises(capi.EpikAmdError, match="42 bits"):
        eplacer.plan_sizes(bins=HEADLINE_BINS, **shape)


def test_what_cannot_take_it_is_refused_when_forced(monkeypatch):
    _clear(monkeypatch)
    monkeypatch.setenv("EPIK_AMD_LAYOUT", "tripled")
    monkeypatch.setenv("EPIK_AMD_RUNS", "1")
    with pytest.raises(capi.EpikAmdError, match="k >= 3"):
        eplacer.plan_sizes(states="nucl", kmer_size=2, num_branches=119, bins=[(5, 10, 10)])
    with pytest.raises(capi.EpikAmdError, match="all runs"):
        eplacer.plan_sizes(states="nucl", kmer_size=5, num_branches=119, bins=[(5, 10, 9)])
    with pytest.raises(capi.EpikAmdError, match="4-letter"):
        eplacer.plan_sizes(states="amino", kmer_size=3, num_branches=119, bins=[(5, 10, 10)])
    with pytest.raises(capi.EpikAmdError, match="shard"):
        eplacer.plan_sizes(states="nucl", kmer_size=5, num_branches=119, bins=[(5, 10, 10)], shard_index=1, shard_count=3)
    with pytest.raises(capi.EpikAmdError, match="one-wavefront"):
        eplacer.plan_sizes(states="nucl", kmer_size=5, num_branches=9999, bins=[(5, 10, 10)])
    monkeypatch.setenv("EPIK_AMD_RUNS", "0")
    with pytest.raises(capi.EpikAmdError, match="run-coded"):
        eplacer.plan_sizes(states="nucl", kmer_size=5, num_branches=119, bins=[(5, 10, 10)])
