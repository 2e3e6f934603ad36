#!/usr/bin/env python3
"""Stage times of the eigenvalues-only call (ek_hip_eigenvalues_device) beside the full call (ek_hip_solve_device)
on the same device-generated inputs, in one process (tools, not product).

  python tools/values_timing.py [--reps R] [--sizes 4096s,16384g,32768g]

Per configuration: one warm-up of each, then R calls of each, best by wall clock (the call synchronises); the stage
seconds printed are the device-event times of that best call.  Then the bisection stage alone (ek_hip_stebz on a
random tridiagonal of order 16384, host arrays: its 256 KB of copies are in the time) for every lane count, for all
indices and for one index -- one index is a single chain of Sturm counts, so its time over the passes is the latency
of one count of length n."""
import argparse
import ctypes
import json
import math
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


def run_config(lib, n, gep, reps):
    keep = []
    dA, dw = dev_alloc(lib, n * n * 8, keep), dev_alloc(lib, n * 8, keep)
    dB = dev_alloc(lib, n * n * 8, keep) if gep else None
    out = {}
    for kind in ("values", "full"):
        dZ = dev_alloc(lib, n * n * 8, keep) if kind == "full" else None
        best = None
        for r in range(reps + 1):
            assert lib.ek_hip_synth_matrix_device(n, 1, dA, n) == 0
            if gep:
                assert lib.ek_hip_synth_matrix_device(n, 2, dB, n) == 0
            st = np.zeros(8)
            t0 = time.perf_counter()
            if kind == "values":
                info = lib.ek_hip_eigenvalues_device(1 if gep else 0, n, 1, n, dA, n, dB, n, dw, st.ctypes.data_as(_dp), 8)
            else:
                info = lib.ek_hip_solve_device(1 if gep else 0, n, n, dA, n, dB, n, dw, dZ, n, st.ctypes.data_as(_dp), 8)
            t = time.perf_counter() - t0
            assert info == 0, (kind, n, info)
            if r > 0 and (best is None or t < best[0]):
                best = (t, st.copy())
        out[kind] = {"wall_s": round(best[0], 4), "stages_s": {k: round(float(v), 4) for k, v in zip(STAGES, best[1])}}
        if dZ is not None:
            lib.ek_hip_free(dZ); keep.remove(dZ)
    for p in keep:
        lib.ek_hip_free(p)
    lib.ek_hip_finalize()
    out["ratio_values_over_full"] = round(out["values"]["wall_s"] / out["full"]["wall_s"], 3)
    return out


def passes_for(d, e, bits):
    """the number of passes stebz_prep gives every index (mirrors ek_stebz.hip)"""
    n = d.shape[0]
    r = np.abs(np.concatenate([[0.0], e])) + np.abs(np.concatenate([e, [0.0]]))
    gl, gu = float((d - r).min()), float((d + r).max())
    pivmin = 2.2250738585072014e-308 * max(1.0, float((e * e).max()) if e.size else 1.0)
    eps = 2.0 ** -53
    tnorm = max(abs(gl), abs(gu))
    gl -= 2.1 * tnorm * eps * n + 4.2 * pivmin
    gu += 2.1 * tnorm * eps * n + 2.1 * pivmin
    tol = 4 * eps * tnorm + 2 * pivmin
    return int(math.ceil(math.log2((gu - gl) / tol) / bits)) if gu - gl > tol else 0


def stebz_alone(lib, n, reps):
    rng = np.random.default_rng(5)
    d, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    w = np.zeros(n)
    rows = []
    for lanes in (1, 2, 4, 8, 16):
        assert lib.ek_hip_debug_set_stebz(lanes) == 0
        res = {}
        for label, il, iu in (("all", 1, n), ("one", n // 2, n // 2)):
            best = 1e30
            for r in range(reps + 1):
                t0 = time.perf_counter()
                assert lib.ek_hip_stebz(n, d.ctypes.data_as(_dp), e.ctypes.data_as(_dp), il, iu, w.ctypes.data_as(_dp)) == 0
                t = time.perf_counter() - t0
                if r > 0:
                    best = min(best, t)
            res[label] = best
        bits = int(math.log2(2 * lanes))
        p = passes_for(d, e, bits)
        rows.append({"lanes": lanes, "points_per_pass": 2 * lanes, "passes": p, "all_indices_s": round(res["all"], 5),
                     "one_index_s": round(res["one"], 5),
                     "one_count_us": round(res["one"] / max(p, 1) * 1e6, 2),
                     "ns_per_pivot_step": round(res["one"] / max(p, 1) / n * 1e9, 2)})
    assert lib.ek_hip_debug_set_stebz(0) == 0
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="4096s,16384g,32768g")
    ap.add_argument("--stebz-n", type=int, default=16384)
    args = ap.parse_args()
    lib = solver.load_library()
    assert lib.ek_hip_init(0) == 0
    result = {"stebz_alone_n%d" % args.stebz_n: stebz_alone(lib, args.stebz_n, args.reps)}
    print(json.dumps(result), flush=True)
    for spec in args.sizes.split(","):
        n, gep = int(spec[:-1]), spec[-1] == "g"
        r = run_config(lib, n, gep, args.reps)
        print(json.dumps({"n": n, "problem": "generalized" if gep else "standard", **r}), flush=True)


if __name__ == "__main__":
    main()
