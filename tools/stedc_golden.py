#!/usr/bin/env python3
"""Records tests/golden/stedc_oracle_spectra.npz: the eigenvalues the CPU oracle's divide & conquer (oracle.stedc) gives for
every class of tests/stedc_cases.py at the orders where the oracle's plain-C products take from seconds to most of a minute
(1100 and 2100).  tests/test_gpu_stedc.py compares the GPU stage with these instead of running the oracle again for every
case; tests/test_stedc_cases_host.py holds the file to a fresh run of the oracle at 1100 and to DSTEBZ at both orders.

    python tools/stedc_golden.py            # about two minutes of CPU
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stedc_cases as sc                 # noqa: E402
from oracle import ek_oracle             # noqa: E402


def main():
    out = {}
    for n in sc.RECORDED_ORDERS:
        for name in sc.CLASSES:
            d, e = sc.tridiagonal(name, n)
            w, _ = ek_oracle.stedc(d, e)
            out["%s_%d" % (name, n)] = w
            print(name, n, flush=True)
    np.savez(sc.RECORDED_PATH, **out)


if __name__ == "__main__":
    main()
