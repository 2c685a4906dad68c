#!/usr/bin/env python3
"""The build record of the kernels of some files: per kernel its VGPRs, SGPRs, spills, static LDS and scratch, read from the
gfx950 ISA listings that `make -C epik_amd/csrc` keeps beside its objects (the metadata the compiler writes for the loader).

    python tools/kernel_figures.py permanova_place permdisp_place edgetest_place model_place [--out FILE] [--build DIR]

Prints one JSON object {file: {kernel (demangled): [vgprs, sgprs, vgpr_spills, sgpr_spills, static_lds, scratch]}}.
profiles/strata_kernels.json holds two of them for the four permutation tests' files, "parent" and "this": the commit before
the strata rule and the one with it, which tests/test_strata_cpu.py compares the build at hand with.
"""
import argparse
import json
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def figures(listing: str) -> dict:
    with open(listing) as fh:
        text = fh.read()
    text = text[text.index("amdhsa.kernels:"):]
    blocks = re.split(r"\n  - (?=\.)", text)[1:]
    names = [re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks]
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(anonymous namespace\)::", "", plain[k]): [int(re.search(rf"\.{f}:\s+(\d+)", b).group(1)) for f in FIELDS]
            for k, b in enumerate(blocks)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--build", default=os.path.join(ROOT, "epik_amd", "csrc", "build", "lib"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    result = {name: figures(os.path.join(args.build, f"{name}-hip-amdgcn-amd-amdhsa-gfx950.s")) for name in args.files}
    line = json.dumps(result, indent=1, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
