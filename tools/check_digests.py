#!/usr/bin/env python3
"""sha256 of what the batched checks on the matrix cores return (the allocations of out and ipr) for the cases of
tests/test_gpu_check_digests.py.  Run on a build whose results are the reference and keep the output: the fixture in the
repository was written on a build of the commit before ek_batched_check_x.h held the shared pieces, in a
worktree of its own, as
    python tools/check_digests.py <that worktree>/eigenkernel_amd/csrc/libek_hip.so > tests/golden/check_digests.txt
Without an argument the library of this tree is taken."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_check_digests as t     # noqa: E402
from eigenkernel_amd import solver     # noqa: E402

lib = solver.load_library(sys.argv[1]) if len(sys.argv) > 1 else solver.load_library()
assert lib.ek_hip_init(0) == 0
print("# <call>  sha256 of the allocations of out and ipr; see tests/test_gpu_check_digests.py")
for case in t.digest_cases():
    print("%s  %s" % (case[0], t.digest_of(lib, case)), flush=True)
