#!/usr/bin/env python3
"""Wall and stage times of the eigenpair windows (ek_hip_eigenpairs_device, RANGE = 'I' and 'V') beside the full call
(ek_hip_solve_device) and the *_select arm that reaches the same window from the bottom (n_vec = iu), on the same
device-generated inputs, in one process (tools, not product).

  python tools/window_timing.py [--reps R] [--sizes 16384g,4096s]
  python tools/window_timing.py --once 16384g      (a warm-up of each, then one 'I' and one 'V' window call: for a
                                                    kernel trace)

A window is m = n / 16 pairs from il = 15 n / 32 + 1 (N = 16384: 1024 pairs at 7681).  The value window's bounds are
the midpoints of the gaps at its ends (from an eigenvalues-only call), so it holds the same pairs.  Per configuration:
one warm-up of each kind, then R rounds that alternate the kinds, best by wall clock (every call synchronises); the
stage seconds printed are the device-event times of that best call."""
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


def window_of(n):
    m = n // 16
    il = 15 * n // 32 + 1
    return il, il + m - 1


def run_config(lib, n, gep, reps, once=False):
    keep = []
    problem = 1 if gep else 0
    dA, dw = dev_alloc(lib, n * n * 8, keep), dev_alloc(lib, n * 8, keep)
    dB = dev_alloc(lib, n * n * 8, keep) if gep else None
    dZ = dev_alloc(lib, n * n * 8, keep)
    il, iu = window_of(n)

    def synth():
        assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
        if gep:
            assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0

    # the value window's bounds: midpoints of the gaps at the index window's ends
    synth()
    assert lib.ek_hip_eigenvalues_device(problem, n, il - 1, iu + 1, dA, n, dB, n, dw, None, 0) == 0
    ends = np.zeros(iu - il + 3)
    assert lib.ek_hip_memcpy_d2h(ends.ctypes.data, dw, ends.nbytes) == 0
    vl, vu = 0.5 * (ends[0] + ends[1]), 0.5 * (ends[-2] + ends[-1])

    def call(kind, st):
        m, f = ctypes.c_int(0), ctypes.c_int(0)
        stp = st.ctypes.data_as(_dp)
        if kind == "window_I":
            info = lib.ek_hip_eigenpairs_device(problem, 1, 0, n, 0.0, 0.0, il, iu, dA, n, dB, n, ctypes.byref(m),
                                                ctypes.byref(f), dw, dZ, n, n, stp, 8)
        elif kind == "window_V":
            info = lib.ek_hip_eigenpairs_device(problem, 1, 1, n, vl, vu, 0, 0, dA, n, dB, n, ctypes.byref(m),
                                                ctypes.byref(f), dw, dZ, n, n, stp, 8)
        elif kind == "select_iu":
            info = lib.ek_hip_solve_device(problem, n, iu, dA, n, dB, n, dw, dZ, n, stp, 8)
            m.value, f.value = iu, 1
        else:
            info = lib.ek_hip_solve_device(problem, n, n, dA, n, dB, n, dw, dZ, n, stp, 8)
            m.value, f.value = n, 1
        return info, m.value, f.value

    kinds = ("window_I", "window_V") if once else ("window_I", "window_V", "select_iu", "full")
    best = {}
    for r in range(1 if once else reps + 1):
        for kind in kinds:
            synth()
            st = np.zeros(8)
            t0 = time.perf_counter()
            info, m, f = call(kind, st)
            t = time.perf_counter() - t0
            assert info == 0, (kind, n, info)
            if kind.startswith("window"):
                assert (m, f) == (iu - il + 1, il), (kind, m, f)
            if r > 0 and (kind not in best or t < best[kind][0]):
                best[kind] = (t, st.copy())
    if once:
        for kind in kinds:
            synth()
            info, _, _ = call(kind, np.zeros(8))
            assert info == 0
    for p in keep:
        lib.ek_hip_free(p)
    lib.ek_hip_finalize()
    if once:
        return {}
    out = {"il": il, "iu": iu, "m": iu - il + 1, "vl": vl, "vu": vu}
    for kind, (t, st) in best.items():
        out[kind] = {"wall_s": round(t, 4), "stages_s": {k: round(float(v), 4) for k, v in zip(STAGES, st)}}
    for kind in ("window_I", "window_V", "select_iu"):
        out["ratio_%s_over_full" % kind] = round(best[kind][0] / best["full"][0], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="16384g,4096s")
    ap.add_argument("--once", default=None, help="one configuration (e.g. 16384g): warm-ups, then one call of each window")
    args = ap.parse_args()
    lib = solver.load_library()
    assert lib.ek_hip_init(0) == 0
    if args.once:
        run_config(lib, int(args.once[:-1]), args.once[-1] == "g", 0, once=True)
        return
    for spec in args.sizes.split(","):
        n, gep = int(spec[:-1]), spec[-1] == "g"
        r = run_config(lib, n, gep, args.reps)
        print(json.dumps({"n": n, "problem": "generalized" if gep else "standard", **r}), flush=True)


if __name__ == "__main__":
    main()
