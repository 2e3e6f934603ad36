#!/usr/bin/env python3
"""sha256 of what the batched window entries return (info, m and the allocations of w, Z, A, B) for the cases of
tests/test_gpu_window_digests.py, each in the device-pointer form and ("<label> host") in the host-pointer form.  Run on a
build whose results are the reference and keep the output: the fixture in the repository was written on a build of the
commit before the solver's host side became one driver, in a worktree of its own, as
    python tools/window_digests.py <that worktree>/eigenkernel_amd/csrc/libek_hip.so > tests/golden/window_digests.txt
Without an argument the library of this tree is taken.  A variable call is run the three ways of the test, which must
agree before its line is written."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_window_digests as t    # noqa: E402
from eigenkernel_amd import solver     # noqa: E402

lib = solver.load_library(sys.argv[1]) if len(sys.argv) > 1 else solver.load_library()
assert lib.ek_hip_init(0) == 0
print("# <call>  sha256 of info, m and of the allocations of w, Z, A, B; see tests/test_gpu_window_digests.py")
for case in t.digest_cases():
    digest = t.digest_of(lib, case)
    if case[1]:
        for tag, budget, streams in t.WAYS:
            assert t.digest_of(lib, case, budget=budget, streams=streams) == digest, (case[0], tag)
    print("%s  %s" % (case[0], digest), flush=True)
    print("%s host  %s" % (case[0], t.digest_of(lib, case, host=True)), flush=True)
