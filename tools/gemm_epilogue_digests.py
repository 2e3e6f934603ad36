#!/usr/bin/env python3
"""sha256 of C after one uniform product per GEMM kernel, transposition and epilogue shape (alpha = -1, beta = 1): the
cases and data of tests/test_gpu_gemm_epilogue.py.  Run on a build whose results are the reference (the fixture in the
repository was written on the commit before the batched epilogue) and keep the output:
    python tools/gemm_epilogue_digests.py > tests/golden/gemm_epilogue_digests.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_gemm_epilogue as t   # noqa: E402
from eigenkernel_amd import solver   # noqa: E402

lib = solver.load_library()
assert lib.ek_hip_init(0) == 0
print("# <kernel> <shape> <ta><tb> K=<k>  sha256 of C's allocation; see tests/test_gpu_gemm_epilogue.py")
for case in t.digest_cases():
    print("%s  %s" % (case[0], t.digest_of(lib, case)), flush=True)
