"""What the deferred tail must not cost the placement kernel, read from the ISA the library was linked from (csrc/Makefile
keeps the listings): the headline instantiation with the tail deferred, place_reads_kernel<DeferredTail<RunListLayout<3,
near, slack>>, uint16_t>, keeps the ring stage of the plain one (at most 13 instructions between two ring loads), its 96
registers and no more scratch; its epilogue is shorter than the plain one's; finish_rows_kernel uses no scratch.  And
the reporter is part of the library's interface."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "epik_amd", "csrc", "build", "lib")
PLACE = os.path.join(BUILD, "place_kernel-hip-amdgcn-amd-amdhsa-gfx950.s")
TAIL = os.path.join(BUILD, "tail_kernel-hip-amdgcn-amd-amdhsa-gfx950.s")
PLAIN = r"place_reads_kernelINS_12_GLOBAL__N_113RunListLayoutILi3ELb1ELb1EEEtEE"
DEFERRED = r"place_reads_kernelINS_12_GLOBAL__N_112DeferredTailINS\d_13RunListLayoutILi3ELb1ELb1EEEEEtEE"


def _lint():
    spec = importlib.util.spec_from_file_location("lint_ring_asm", os.path.join(ROOT, "epik_amd", "csrc", "lint_ring_asm.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    return lint


def _kernels(path):
    text = open(path).read()
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        field = lambda k: int(re.search(r"\.amdhsa_" + k + r"\s+(\d+)", m.group(2)).group(1))
        yield m.group(1), field("next_free_vgpr"), field("private_segment_fixed_size")


def _function_lengths(path, name_re):
    """Instructions of every function of the listing whose name matches."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_ZN\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", text, re.S | re.M):
        if re.search(name_re, m.group(1)):
            out[m.group(1)] = sum(1 for l in m.group(2).split("\n") if l.startswith("\t") and not l.startswith("\t."))
    return out


def _need_listings():
    from epik_amd import capi
    assert os.path.exists(capi.LIB_PATH), "build the library first (python3 __graft_entry__.py)"
    for path in (PLACE, TAIL):
        assert os.path.exists(path), f"the library is built but the listing it was linked from is missing: {path}"


def test_the_deferred_headline_kernel_keeps_the_ring_stage_and_the_registers():
    _need_listings()
    lint = _lint()
    plain, deferred = lint.ring_stages(PLACE, PLAIN), lint.ring_stages(PLACE, DEFERRED)
    assert len(plain) == 1 and len(deferred) == 1, (sorted(plain), sorted(deferred))
    (kernel, stages), (_, before) = next(iter(deferred.items())), next(iter(plain.items()))
    assert len(stages["loops"]) == 1
    gaps = stages["loops"][0]
    assert len(gaps) == 7, f"{kernel}: eight ring loads a trip expected, found {len(gaps) + 1}"
    for n, gap in enumerate(gaps):
        assert gap["total"] <= 13, (n, gap)
        assert gap.get("salu", 0) <= 4 and gap.get("valu", 0) <= 4, (n, gap)
        assert gap.get("nop", 0) == 0 and gap.get("branch", 0) == 0, (n, gap)
    assert stages["scratch"] is not None and stages["scratch"] <= before["scratch"], (stages["scratch"], before["scratch"])
    regs = {name: (vgpr, scratch) for name, vgpr, scratch in _kernels(PLACE)}
    seen = 0
    for name, (vgpr, scratch) in regs.items():
        if "DeferredTail" in name:
            twin = re.sub(r"12DeferredTailINS\d_(13RunListLayoutI(?:L[ib]\dE)+E)EE", r"\1", name)  # the same kernel over the plain layout
            assert twin in regs, (name, twin)
            assert vgpr <= 96 and scratch <= regs[twin][1], (name, vgpr, scratch, regs[twin])
            seen += 1
    assert seen >= 4   # the tripled table alone: slack rows or the clamp, 16- and 32-bit counts


def test_the_deferred_epilogue_is_the_shorter_one():
    _need_listings()
    plain = _function_lengths(PLACE, r"place_epilogueINS\d_13RunListLayoutILi3ELb1ELb1EEEt")
    deferred = _function_lengths(PLACE, r"place_epilogueINS\d_12DeferredTailINS\d_13RunListLayoutILi3ELb1ELb1EEEEEt")
    assert len(plain) == 1 and len(deferred) == 1, (sorted(plain), sorted(deferred))
    (a,), (b,) = plain.values(), deferred.values()
    print(f"epilogue of the headline instantiation: {a} instructions with the tail, {b} without")
    assert b < a - 300, (a, b)   # an exp10, two double divisions and the filter are gone: several hundred instructions


def test_the_finishing_kernel_needs_no_scratch():
    _need_listings()
    groups = {}
    for name, vgpr, scratch in _kernels(TAIL):
        m = re.match(r"_ZN8epik_amd18finish_rows_kernelILj(\d+)EEE", name)
        if m:
            groups[int(m.group(1))] = (vgpr, scratch)
    assert sorted(groups) == [1, 2, 4, 8, 16, 32, 64], sorted(groups)
    for g, (vgpr, scratch) in groups.items():
        assert scratch == 0 and vgpr <= 64, (g, vgpr, scratch)


def test_the_reporter_is_exported_and_documented():
    from epik_amd import capi
    assert "epik_amd_placer_tail_form" in capi.EXPORTS
    assert (capi.TAIL_WAVE, capi.TAIL_KERNEL) == (0, 1)
    header = open(os.path.join(ROOT, "include", "epik_amd.h")).read()
    assert "int epik_amd_placer_tail_form(const epik_amd_placer *p, uint32_t counts, uint32_t *form);" in header
    assert "#define EPIK_AMD_TAIL_KERNEL 1u" in header and "#define EPIK_AMD_TAIL_WAVE 0u" in header
    if os.path.exists(capi.LIB_PATH):
        assert hasattr(capi.load(), "epik_amd_placer_tail_form")
