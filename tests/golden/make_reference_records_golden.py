#!/usr/bin/env python3
"""Generates tests/golden/reference_records.json: what two pieces of the reference's own Python say about the
inputs of tests/test_host_cpu.py, so that those tests run from this repository alone.

  launcher       -- the argv the reference's `place_queries` (epik.py) hands to subprocess.call for the two
                    cases of test_launcher_argv_equals_the_reference_launcher (the binary as its base name:
                    its directory is the install's);
  legacy_differ  -- the pairs of jplace documents of test_legacy_differ_agrees_with_the_reference_script and
                    how many names the reference's comparison function (scripts/jplace_diff.py) matched on each,
                    with and without only_best.

The fixture holds inputs and the reference's outputs only (data, no reference text).  Run it where a checkout
of the reference is present, with that checkout's path:

    python tests/golden/make_reference_records_golden.py PATH_TO_REFERENCE
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from epik_amd import jplace  # noqa: E402

# (states, max_ram) of the launcher cases; the other arguments are the test's
LAUNCHER_CASES = [("nucl", None), ("amino", "4G")]


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_pair():
    """Seeded jplace contents with every kind of disagreement (the pairs the test used to build itself)."""
    rng = np.random.default_rng(7)
    names = [f"s{i}" for i in range(60)]

    def rows(n):
        edges = rng.choice(40, size=n, replace=False)
        return [dict(edge_num=int(e), likelihood=float(-rng.uniform(0.5, 6.0)), like_weight_ratio=float(rng.random()),
                     distal_length=0.1, pendant_length=0.2) for e in edges]

    first = {name: rows(int(rng.integers(0, 6))) for name in names}
    second = json.loads(json.dumps(first))
    for i, name in enumerate(names):
        r = second[name]
        kind = i % 6
        if kind == 1 and r:
            r[0]["likelihood"] += 5e-5           # inside the 1e-4 window
        elif kind == 2 and r:
            r[0]["likelihood"] -= 0.5            # outside: compared edge by edge on 10**likelihood
        elif kind == 3 and r:
            r[0]["edge_num"] = 99                # another edge with the same likelihood: still a "match" there
        elif kind == 4 and r:
            r.pop()                              # a row missing
        elif kind == 5:
            r.append(dict(edge_num=77, likelihood=-9.0, like_weight_ratio=0.0, distal_length=0.0, pendant_length=0.0))
    return first, second


def write(path, placed):
    doc = {"fields": jplace.FIELDS, "version": 3, "tree": "(A:1{0},B:2{1}):0{2};", "metadata": {},
           "placements": [{"p": [[r[f] for f in jplace.FIELDS] for r in rws], "nm": [[name, 1]]}
                          for name, rws in placed.items()]}
    with open(path, "w") as fh:
        json.dump(doc, fh)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    reference = sys.argv[1]
    ref_epik = load(os.path.join(reference, "epik.py"), "reference_epik")
    launcher = []
    for states, max_ram in LAUNCHER_CASES:
        seen = []
        with mock.patch.object(ref_epik.subprocess, "call", lambda command: seen.append(list(command)) or 0), \
                contextlib.redirect_stdout(io.StringIO()):
            ref_epik.place_queries("db.ipk", states, 1.5, 0.8, "out", 3, max_ram, "q.fasta")
        argv = [os.path.basename(seen[0][0])] + seen[0][1:]
        launcher.append({"states": states, "max_ram": max_ram, "argv": argv})

    ref_diff = load(os.path.join(reference, "scripts", "jplace_diff.py"), "reference_jplace_diff")
    first, second = make_pair()
    matched = {}
    with tempfile.TemporaryDirectory() as tmp:
        a, b = os.path.join(tmp, "a.jplace"), os.path.join(tmp, "b.jplace")
        write(a, first)
        write(b, second)
        for only_best in (False, True):
            out = io.StringIO()
            with contextlib.redirect_stdout(out):
                ref_diff.jplace_diff.callback(a, b, only_best)
            matched[str(only_best).lower()] = int(out.getvalue().strip().splitlines()[-1].split("/")[0])

    with open(os.path.join(HERE, "reference_records.json"), "w") as fh:
        json.dump({"generator": "tests/golden/make_reference_records_golden.py",
                   "launcher": {"reference": "epik.py: place_queries(), the argv given to subprocess.call",
                                "call": {"database": "db.ipk", "omega": 1.5, "mu": 0.8, "outputdir": "out", "threads": 3,
                                         "input_file": "q.fasta"},
                                "cases": launcher},
                   "legacy_differ": {"reference": "scripts/jplace_diff.py: jplace_diff(), EPSILON = 1e-4 on 10**likelihood",
                                     "first": first, "second": second, "names": len(first),
                                     "reference_matched": matched}}, fh)
    print(launcher, matched)


if __name__ == "__main__":
    main()
