"""The database-building kernels at their seams: every case of test_build_seams_cpu.py through the
device -- build_place.hip's merge paths on planted ghost nodes with a finish after every chunk, its grid-stride loops on a
chunk of 2^20 + 300 ghost nodes and more than 4 194 304 tuples (through `add` and `add_device`), its deepest walks at
k = 15 and amino k = 7 over a full tile, the packed word at N up to 2^32 - 1 with the highest key, both ways a chunk is
found too large and the refusal's byte count, log_thr = -inf and either zero; filter_place.hip's second sweep over
2^21 + 65 keys; and ancestral_place.hip's chunked output written straight into a poisoned device array.  Bytes equal to
the expectation the CPU file has checked the host mirror against."""
import re

import numpy as np
import pytest

from epik_amd import ancestral, build, capi, filters
from test_ancestral_cpu import get_case as ancestral_case
from test_ancestral_cpu import same_posteriors
from test_ancestral_gpu import site_bytes
from test_build_seams_cpu import (ANCESTRAL_CHUNK_SITES, ANCESTRAL_SEAM_CASES, BUILD_ELEMENTS_CAP, BUILD_UNITS_CAP, DEEP_CASES, MERGE_N,
                                  MERGE_SCENARIOS, PLANT_THR, TUPLE_BYTES, WIDTH_ALPHABETS, WIDTH_N, ancestral_want, check_best_kmers,
                                  check_merge_path, deep_case, deep_expectation, deep_rounding_case, deep_rounding_thresholds, host_of,
                                  items_route_case, joined, log_thr_case, merge_chunks, merge_stages, numpy_of, once, partial_case,
                                  planted_host, refusal_cases, sliced, stride_build_case, stride_build_host, stride_build_stages, stride_filter_case,
                                  stride_filter_host, tuples_route_case, width_case)
from test_dbbuild_cpu import same_db
from test_filter_cpu import same_bytes
from test_filter_gpu import rank_on_stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device(gpu_available):
    assert gpu_available, "pytest -m gpu needs a HIP device (no CPU fallback exists)"


def builder_for(case, **kw):
    return build.Builder(case["states"], case["k"], case["N"], log_thr=case["log_thr"], **kw)


def planted_builder(num_branches, **kw):
    return build.Builder("nucl", 2, num_branches, log_thr=PLANT_THR, **kw)


def on_device(case):
    import torch
    return torch.from_numpy(case["logp"]).cuda(), torch.from_numpy(case["branch_of"].view(np.int32)).cuda()


def built(case, device_entry=False, **kw):
    """(the database, num_splits) of one chunk through `add` or `add_device`."""
    with builder_for(case, **kw) as b:
        if device_entry:
            b.add_device(*on_device(case))
        else:
            b.add(case["logp"], case["branch_of"])
        return b.finish(), b.num_splits


# ---- 2. the paths of the merge ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MERGE_SCENARIOS))
def test_merge_paths_with_a_finish_after_every_chunk(name):
    chunks, stages = merge_chunks(name), merge_stages(name)
    got = []
    with planted_builder(MERGE_N) as b:
        for i, (logp, branch_of) in enumerate(chunks):
            b.add(logp, branch_of)
            got.append(b.finish())
            same_db(got[-1], stages[i])
            same_db(got[-1], planted_host(MERGE_N, joined(chunks[:i + 1])))
        assert b.num_splits == 0
    check_merge_path(name, got)


# ---- 3. grid strides ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("device_entry", [False, True], ids=["add", "add_device"])
def test_every_grid_stride_of_the_builder(device_entry):
    """2^20 + 300 ghost nodes of one tile each (enumerate_kernel strides), 4 x that many tuples, all distinct pairs (head_flag,
    reduce, merge_write and csr stride), a second chunk that searches and rewrites that store (merge_rank, merge_write), and
    8 x that many logp values through add_device (validate strides)."""
    import torch
    case, stages = stride_build_case(), stride_build_stages()
    first = case["chunks"][0]
    assert first[0].shape[0] > BUILD_UNITS_CAP and len(stages[0].values) > BUILD_ELEMENTS_CAP and first[0].size > BUILD_ELEMENTS_CAP
    with planted_builder(case["N"]) as b:
        for i, (logp, branch_of) in enumerate(case["chunks"]):
            if device_entry:
                b.add_device(torch.from_numpy(logp).cuda(), torch.from_numpy(branch_of.view(np.int32)).cuda())
            else:
                b.add(logp, branch_of)
            same_db(b.finish(), stages[i])
        assert b.num_splits == 0
    same_db(stride_build_host(), stages[1])


def test_the_second_sweep_of_the_filter_grid():
    """2^21 + 65 keys: 32 770 tiles for 32 768 waves, so two tiles are reached by `tile += waves` alone; they hold long lists
    and the smallest and largest images, so the sorted bit range needs `low` / `high` carried across the stride."""
    c = stride_filter_case()
    assert (len(c["keys"]) + 63) // 64 > 8192 * 4
    for name in filters.FILTERS:
        got = rank_on_stream(c["N"], c["log_thr"], c["keys"], c["offsets"], c["values"], name, 9)
        assert same_bytes(got, stride_filter_host(name)), name


# ---- 4. the deepest and widest walks ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(DEEP_CASES))
def test_deep_walks(name):
    case, want = deep_case(name), deep_expectation(name)
    assert 10 ** 4 <= want.num_entries <= 2 * 10 ** 6
    db, splits = built(case)
    same_db(db, want)
    check_best_kmers(case, db)
    assert splits == 0


def test_deep_rounding_and_the_threshold_seam():
    case = deep_rounding_case()
    base, at, above = deep_rounding_thresholds()
    same_db(built(case)[0], base)
    for thr in (at, above):
        case["log_thr"] = thr
        db = built(case)[0]
        same_db(db, host_of(case))
        assert db.num_entries == base.num_entries - (0 if thr == at else int((base.values["score"] == at).sum()))


# ---- 5. the width of the packed word ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", WIDTH_N)
@pytest.mark.parametrize("states,k", WIDTH_ALPHABETS)
def test_width_of_the_packed_word(states, k, N):
    case, want = width_case(states, k, N)
    with builder_for(case) as b:
        b.add(case["logp"], case["branch_of"])
        db = b.finish()
        same_db(db, want)
        for name in ("best", "mif0"):
            assert same_bytes(b.rank(name), filters.rank_host(N, db.log_threshold, db.keys, db.offsets, db.values, name)), name
        b.add_device(*on_device(case))                                   # (the same pairs again: nothing may change)
        same_db(b.finish(), want)


# ---- 6. workspaces, splits and the partial add ---------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["items", "tuples"])
@pytest.mark.parametrize("device_entry", [False, True], ids=["add", "add_device"])
def test_both_ways_a_chunk_is_found_too_large(route, device_entry):
    case, ws = items_route_case() if route == "items" else tuples_route_case()
    want = once("route-" + route, lambda: host_of(case, num_threads=4))
    whole, no_splits = built(case, device_entry)
    split, splits = built(case, device_entry, workspace_bytes=ws)
    assert no_splits == 0 and splits > 0 and want.num_entries > 0
    same_db(whole, want)
    same_db(split, want)


@pytest.mark.parametrize("route", ["items", "tuples"])
def test_the_refusal_names_the_bytes_that_suffice(route):
    chunk, ws, need = refusal_cases()[route]
    message = r"ghost node 0 of the chunk needs a workspace of (\d+) bytes, the builder has %d"
    with builder_for(chunk, workspace_bytes=ws) as b:
        with pytest.raises(capi.EpikAmdError, match=message % ws) as info:
            b.add(chunk["logp"], chunk["branch_of"])
        assert b.finish().num_entries == 0
    X = int(re.search(message % ws, str(info.value)).group(1))
    assert X == need
    db, splits = built(chunk, workspace_bytes=X)
    same_db(db, host_of(chunk))
    assert splits == 0 and db.num_entries > 0
    with builder_for(chunk, workspace_bytes=X - TUPLE_BYTES) as b:
        with pytest.raises(capi.EpikAmdError, match=message % (X - TUPLE_BYTES)) as again:
            b.add_device(*on_device(chunk))
    assert int(re.search(message % (X - TUPLE_BYTES), str(again.value)).group(1)) == X


def test_a_refused_ghost_node_leaves_the_ones_before_it_added():
    case, ws = partial_case()
    with builder_for(case, workspace_bytes=ws) as b:
        with pytest.raises(capi.EpikAmdError, match=r"ghost node 2 of the chunk needs a workspace of \d+ bytes") as info:
            b.add(case["logp"], case["branch_of"])
        assert info.value.code == capi.ERR_INVALID and "the ghost nodes before it were added" in str(info.value)
        same_db(b.finish(), host_of(sliced(case, (0, 1))))
        assert b.num_splits == 2
        b.add(case["logp"][3:], case["branch_of"][3:])
        same_db(b.finish(), host_of(sliced(case, (0, 1, 3))))
    with builder_for(case, workspace_bytes=ws) as b:                      # the same through the device entry
        with pytest.raises(capi.EpikAmdError, match=r"ghost node 2 of the chunk needs a workspace of \d+ bytes"):
            b.add_device(*on_device(case))
        same_db(b.finish(), host_of(sliced(case, (0, 1))))


# ---- 7. log_thr at its ends ------------------------------------------------------------------------------------------------

def test_log_thr_minus_infinity():
    case = log_thr_case(-np.inf)
    want = numpy_of(case)
    with builder_for(case) as b:
        b.add(case["logp"], case["branch_of"])
        db = b.finish()
        same_db(db, want)
        same_db(db, host_of(case))
        assert np.isneginf(db.values["score"]).any()
        for name in filters.FILTERS:
            assert same_bytes(b.rank(name, seed=3), filters.rank_host(case["N"], db.log_threshold, db.keys, db.offsets, db.values, name, seed=3)), name


def test_log_thr_of_either_zero():
    plus, minus = built(log_thr_case(0.0))[0], built(log_thr_case(-0.0))[0]
    same_db(plus, minus)
    same_db(plus, numpy_of(log_thr_case(0.0)))
    assert plus.num_entries > 0 and np.all(plus.values["score"].view(np.uint32) == 0)
    same_db(built(log_thr_case(-0.0), device_entry=True)[0], plus)


# ---- 8. the chunked device output of the ancestral kernels -----------------------------------------------------------------

@pytest.mark.parametrize("sites", ANCESTRAL_CHUNK_SITES)
@pytest.mark.parametrize("name", ANCESTRAL_SEAM_CASES)
def test_chunks_of_sites_written_straight_into_the_device_array(name, sites):
    """posteriors_device writes every chunk of sites at its own place of the caller's [G][L][S] array: a workspace of `sites`
    sites, an array full of 0xA5 before the call, every choice of ghost nodes."""
    import torch
    case = ancestral_case(name)
    L = case["masks"].shape[1]
    with ancestral.Ancestral(*case["inputs"], workspace_bytes=site_bytes(case) * sites + 768) as a:
        for ghosts in ("both", "inner", "outer"):
            want = ancestral_want(name, ghosts)
            out = torch.full(want[0].shape, -0x5A5A5A5B, dtype=torch.int32, device="cuda").view(torch.float32)
            d_post, d_branch_of, dead = a.posteriors_device(case["masks"], ghosts, out=out)
            assert d_post.data_ptr() == out.data_ptr()
            same_posteriors((d_post.cpu().numpy(), d_branch_of.cpu().numpy().view(np.uint32), dead), want)
