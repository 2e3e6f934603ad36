#!/usr/bin/env python3
"""Wall and stage times of DSYGVX's three problem types (ek_hip_sygvx_device: itype 1 A x = l B x, 2 A B x = l x,
3 B A x = l x), with and without eigenvectors, on the same device-generated pair, in one process (tools, not product).

  python tools/sygvx_timing.py [--reps R] [--sizes 16384,4096]

Per order: one warm-up of each (type, jobz), then R rounds that alternate them, best by wall clock (every call
synchronises); the stage seconds printed are the device-event times of that best call: the reduction (L^-1 A L^-T or
L^T A L) in "sygst", the recovery (L^-T y or L y) in "trtrs"."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eigenkernel_amd import solver  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
STAGES = ["potrf", "sygst", "sytrd", "gather", "stedc", "ormtr", "trtrs", "copy"]


def dev_alloc(lib, nbytes, keep):
    p = ctypes.c_void_p()
    assert lib.ek_hip_malloc(ctypes.byref(p), int(nbytes)) == 0
    keep.append(p)
    return p


def run_order(lib, n, reps):
    keep = []
    dA, dB, dZ = (dev_alloc(lib, n * n * 8, keep) for _ in range(3))
    dw = dev_alloc(lib, n * 8, keep)
    kinds = [(it, jobz) for jobz in (1, 0) for it in (1, 2, 3)]
    best = {}
    for r in range(reps + 1):
        for it, jobz in kinds:
            assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
            assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
            assert lib.ek_hip_synchronize() == 0
            st = np.zeros(8)
            m, f = ctypes.c_int(0), ctypes.c_int(0)
            t0 = time.perf_counter()
            info = lib.ek_hip_sygvx_device(it, jobz, 0, n, 0.0, 0.0, 1, n, dA, n, dB, n, ctypes.byref(m),
                                           ctypes.byref(f), dw, dZ, n, n, st.ctypes.data_as(_dp), 8)
            t = time.perf_counter() - t0
            assert info == 0 and m.value == n, (it, jobz, info, m.value)
            key = "itype%d_%s" % (it, "vectors" if jobz else "values")
            if r > 0 and (key not in best or t < best[key][0]):
                best[key] = (t, st.copy())
    for p in keep:
        lib.ek_hip_free(p)
    lib.ek_hip_finalize()
    out = {}
    for key, (t, st) in best.items():
        out[key] = {"wall_s": round(t, 4), "stages_s": {k: round(float(v), 4) for k, v in zip(STAGES, st)}}
    for it in (2, 3):
        out["ratio_itype%d_over_itype1" % it] = round(best["itype%d_vectors" % it][0] / best["itype1_vectors"][0], 3)
        out["ratio_itype%d_values_over_itype1" % it] = round(best["itype%d_values" % it][0] / best["itype1_values"][0], 3)
        out["ratio_itype%d_sygst_over_itype1" % it] = round(float(best["itype%d_vectors" % it][1][1]) /
                                                            float(best["itype1_vectors"][1][1]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="16384,4096")
    args = ap.parse_args()
    lib = solver.load_library()
    assert lib.ek_hip_init(0) == 0
    for spec in args.sizes.split(","):
        n = int(spec)
        print(json.dumps({"n": n, **run_order(lib, n, args.reps)}), flush=True)


if __name__ == "__main__":
    main()
