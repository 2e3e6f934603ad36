#!/usr/bin/env python3
"""Digests of what the one-problem path returns for the cases of tests/test_gpu_path_digests.py (to compare two builds of
the library bit for bit; EK_HIP_LIB picks the build).  Run on a build whose results are the reference:
    python tools/path_digests.py > tests/golden/path_anchor_digests.txt
Every case runs twice; one whose two lines differ is not written but named on stderr (and belongs into DESIGN.md).
    python tools/path_digests.py --only "<label>"
prints that case's line from one run (how a case whose switch is read once per process is run, twice, by the above)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_path_digests as t      # noqa: E402
from eigenkernel_amd import solver     # noqa: E402
from oracle import ek_oracle           # noqa: E402


def own_process(label):
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--only", label], stdout=subprocess.PIPE,
                          check=True, universal_newlines=True).stdout.strip()


if len(sys.argv) == 3 and sys.argv[1] == "--only":
    assert solver.load_library().ek_hip_init(0) == 0
    print(t.line_of(t.CASES[t.LABELS.index(sys.argv[2])], solver, ek_oracle))
    sys.exit(0)
assert solver.load_library().ek_hip_init(0) == 0
print("# <case>  <switches set for it>  <output>=<first 16 hex digits of its SHA-256> ...; see tests/test_gpu_path_digests.py")
for case in t.CASES:
    if case[3]:
        first, second = own_process(case[0]), own_process(case[0])
    else:
        first, second = t.line_of(case, solver, ek_oracle), t.line_of(case, solver, ek_oracle)
    if first == second:
        print(first, flush=True)
    else:
        print("DROPPED (two runs differ): %s\n  %s\n  %s" % (case[0], first, second), file=sys.stderr, flush=True)
