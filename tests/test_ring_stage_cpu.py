"""The steady-state stage of the run-list ring in the headline kernel, counted in the ISA the library was linked from
(csrc/Makefile keeps the listings; lint_ring_asm.py --stages counts them): place_reads_kernel<RunListLayout<1, near,
slack>, uint16_t> spends at most 13 instructions between two consecutive ring loads of its loop (12 with the load
itself was the aim: 4 VALU, 2 LDS, 3 SALU, the two waits; the far form it replaces took 19), of which at most 4 scalar
and 4 vector ALU, no s_nop and no branch -- and no more scratch than the far form of the same kernel, which is the
kernel the near form replaced."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(ROOT, "epik_amd", "csrc", "build", "lib", "place_kernel-hip-amdgcn-amd-amdhsa-gfx950.s")
HEADLINE = r"place_reads_kernelINS_12_GLOBAL__N_113RunListLayoutILi1ELb1ELb1EEEtEE"
FAR = r"place_reads_kernelINS_12_GLOBAL__N_113RunListLayoutILi1ELb0ELb0EEEtEE"


def _lint():
    spec = importlib.util.spec_from_file_location("lint_ring_asm", os.path.join(ROOT, "epik_amd", "csrc", "lint_ring_asm.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    return lint


def test_the_headline_ring_stage_keeps_its_budget():
    from epik_amd import capi
    assert os.path.exists(capi.LIB_PATH), "build the library first (python3 __graft_entry__.py)"
    # (the library is there: its listing must be too -- a build that does not keep it cannot be checked, and fails here)
    assert os.path.exists(LISTING), f"the library is built but the listing it was linked from is missing: {LISTING}"
    lint = _lint()
    near = lint.ring_stages(LISTING, HEADLINE)
    far = lint.ring_stages(LISTING, FAR)
    assert len(near) == 1 and len(far) == 1, (sorted(near), sorted(far))
    (kernel, stages), (_, before) = next(iter(near.items())), next(iter(far.items()))
    assert len(stages["loops"]) == 1, f"{kernel}: one ring loop expected, found {len(stages['loops'])}"
    gaps = stages["loops"][0]
    assert len(gaps) == 7, f"{kernel}: eight ring loads a trip expected, found {len(gaps) + 1}"
    for n, gap in enumerate(gaps):
        print(f"stage {n}: " + ", ".join(f"{k} {v}" for k, v in gap.items() if k != "ops"))
        assert gap["total"] <= 13, (n, gap)
        assert gap.get("salu", 0) <= 4 and gap.get("valu", 0) <= 4, (n, gap)
        assert gap.get("nop", 0) == 0 and gap.get("branch", 0) == 0, (n, gap)
        assert gap.get("lds", 0) == 2 and gap.get("vmem", 0) == 0 and gap.get("other", 0) == 0, (n, gap)
    assert stages["scratch"] is not None and before["scratch"] is not None
    assert stages["scratch"] <= before["scratch"], (stages["scratch"], before["scratch"])


def test_the_stage_count_reads_conditional_assembly_like_the_assembler(tmp_path):
    """`.if 1 == 0` / `s_nop 4` / `.endif`, as Layout::issue<kSettled> leaves it in the listing, is no instruction;
    with `.if 0 == 0` it is one, and it counts five wait states for the refill behind it."""
    lint = _lint()

    def kernel(flag):
        lines = ["_ZN8epik_amd18place_reads_kernelIcEEvNS_11PlaceParamsE:", ".LBB0_1:"]
        for slot in (6, 7):
            lines += [f"\tds_read_b32 v12, v{slot + 4}", "\t;;#ASMSTART", "\tv_readlane_b32 s9, v2, 0", "\t;;#ASMEND",
                      "\t;;#ASMSTART", "\ts_waitcnt vmcnt(1)", "\t;;#ASMEND", f"\tds_write_b32 v{slot + 4}, v12",
                      "\t;;#ASMSTART", f"\t.if {flag} == 0", "\ts_nop 4", "\t.endif",
                      f"\tbuffer_load_dword v{slot}, v1, s[4:7], s9 offen", "\t;;#ASMEND"]
        lines += ["\ts_cbranch_scc1 .LBB0_1", "\ts_endpgm"]
        path = tmp_path / f"k{flag}.s"
        path.write_text("\n".join(lines) + "\n")
        problems = []
        lint.lint_settled("k", lines[1:], problems)
        (stages,) = lint.ring_stages(str(path), "place_reads_kernel").values()
        return stages["loops"][0][0], problems

    gap, problems = kernel(1)
    assert gap["total"] == 4 and gap.get("nop", 0) == 0
    assert len(problems) == 2   # two instructions between the v_readlane and the load that reads s9: three short
    gap, problems = kernel(0)
    assert gap["total"] == 5 and gap["nop"] == 1 and problems == []
