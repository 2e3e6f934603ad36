#!/usr/bin/env python
"""Triplet entries against the dense host entries, on one GPU.

There is no matrix to download: the tool generates a banded SPD pair (half bandwidth 32) as a triplet list of the lower
triangle, and the dense mirrored matrices from it.  Per order it times, best of 3 with the two forms alternated in one
process:
  ek_hip_solve (dense host arrays, 1 x 1)    against  ek_hip_solve_sparse (the triplets), wall time, with the
      EK_STAGE_COPY part of each and the CSR build of both matrices on its own (ek_hip_debug_sparse_csr);
  the three ek_hip_check calls (residual, orthogonality, IPR on dense host arrays)  against  one ek_hip_check_sparse.
With --host-files DIR it also writes the pair as MatrixMarket files (what the Fortran host reads with and without
--triplets).

    python tools/sparse_timing.py [--sizes 4096,16384] [--bw 32] [--reps 3] [--out profiles/sparse_timing.txt]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from eigenkernel_amd import descriptor as dsc  # noqa: E402
from eigenkernel_amd import solver  # noqa: E402

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_llp = ctypes.POINTER(ctypes.c_longlong)
COPY = 7   # EK_STAGE_COPY


def P(a):
    return a.ctypes.data_as(_dp)


def I(a):
    return a.ctypes.data_as(_ip)


def banded_triplets(n, bw, seed, spd):
    """Lower triangle of a symmetric band: (suffix (nnz, 2) int32 1-based, value).  spd: diagonal 2, off-diagonal row
    sums below 1 (spectrum in [1, 3]); else a diagonal in [3, 5] over the same band (SPD as well)."""
    rng = np.random.default_rng(seed)
    off = np.arange(n, dtype=np.int32)
    rows, cols = [off], [off]
    vals = [np.full(n, 2.0) if spd else rng.uniform(3.0, 5.0, n)]
    for k in range(1, bw + 1):
        rows.append(off[k:]); cols.append(off[:-k])
        vals.append(rng.uniform(-1.0, 1.0, n - k) * 0.5 / bw)
    suf = np.ascontiguousarray(np.stack([np.concatenate(rows), np.concatenate(cols)], axis=1) + 1, dtype=np.int32)
    return suf, np.ascontiguousarray(np.concatenate(vals))


def dense_of(n, suf, val):
    D = np.zeros((n, n), order="F")
    D[suf[:, 0] - 1, suf[:, 1] - 1] = val
    D[suf[:, 1] - 1, suf[:, 0] - 1] = val
    return D


def write_mtx(path, n, suf, val):
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write("%d %d %d\n" % (n, n, val.size))
        np.savetxt(f, np.column_stack([suf, val]), fmt="%d %d %.17e")


def best(xs):
    return min(xs)


def run(n, bw, reps, lines, host_files):
    lib = solver.load_library()
    sa, va = banded_triplets(n, bw, 1, False)
    sb, vb = banded_triplets(n, bw, 2, True)
    nnz = int(va.size)
    if host_files:
        write_mtx(os.path.join(host_files, "band_%d_A.mtx" % n), n, sa, va)
        write_mtx(os.path.join(host_files, "band_%d_B.mtx" % n), n, sb, vb)
    t = time.perf_counter()
    A0, B0 = dense_of(n, sa, va), dense_of(n, sb, vb)
    t_form = time.perf_counter() - t                  # what a host of the dense entries pays first (here: numpy)
    A, B = np.empty_like(A0), np.empty_like(B0)
    desc = dsc.descinit(n, n, 64, 64, 0, 0, 0, n)
    w1, w2 = np.zeros(n), np.zeros(n)
    Z1, Z2 = np.zeros((n, n), order="F"), np.zeros((n, n), order="F")
    st1, st2 = np.zeros(8), np.zeros(8)
    rp = np.zeros(n + 1, dtype=np.int64); ci = np.zeros(2 * nnz, dtype=np.int32); cv = np.zeros(2 * nnz)

    def dense_solve():
        A[...] = A0; B[...] = B0                      # (the call overwrites its matrices: not timed)
        t = time.perf_counter()
        rc = lib.ek_hip_solve(1, n, n, P(A), I(desc), P(B), I(desc), P(w1), P(Z1), I(desc), 1, 1, 0, 0, P(st1), 8)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt, float(st1[COPY])

    def sparse_solve():
        t = time.perf_counter()
        rc = lib.ek_hip_solve_sparse(1, n, n, nnz, I(sa), P(va), nnz, I(sb), P(vb), P(w2), P(Z2), I(desc), 1, 1, 0, 0,
                                     P(st2), 8)
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt, float(st2[COPY])

    def csr_build():
        t = time.perf_counter()
        for s, v in ((sa, va), (sb, vb)):
            m = lib.ek_hip_debug_sparse_csr(n, nnz, I(s), P(v), rp.ctypes.data_as(_llp), I(ci), P(cv))
            assert m > 0, m
        return time.perf_counter() - t

    dense_solve(); sparse_solve()                      # workspaces grown, kernels loaded, pages touched
    td, ts, tc = [], [], []
    for _ in range(reps):
        td.append(dense_solve()); ts.append(sparse_solve()); tc.append(csr_build())
    assert w1.tobytes() == w2.tobytes() and Z1.tobytes() == Z2.tobytes(), "the two solves differ"
    d, s = min(td), min(ts)

    out_d, out_s = np.zeros(max(n, 3)), np.zeros(4)
    ipr_d, ipr_s = np.zeros(n), np.zeros(n)

    def dense_check():
        t = time.perf_counter()
        rc = lib.ek_hip_check(0, 1, n, n, 1, n, P(A0), I(desc), P(B0), I(desc), P(w1), P(Z1), I(desc), P(out_d))
        res = out_d[:3].copy()
        rc |= lib.ek_hip_check(1, 1, n, 0, 1, n, None, None, P(B0), I(desc), P(w1), P(Z1), I(desc), P(out_d))
        orth = float(out_d[0])
        rc |= lib.ek_hip_check(2, 1, n, n, 1, n, None, None, P(B0), I(desc), P(w1), P(Z1), I(desc), P(ipr_d))
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt, np.append(res, orth)

    def sparse_check():
        t = time.perf_counter()
        rc = lib.ek_hip_check_sparse(1, n, nnz, I(sa), P(va), nnz, I(sb), P(vb), P(w1), P(Z1), n, n, 1, n, n, P(out_s),
                                     P(ipr_s))
        dt = time.perf_counter() - t
        assert rc == 0, rc
        return dt, out_s.copy()

    dense_check(); sparse_check()
    cd, cs = [], []
    for _ in range(reps):
        cd.append(dense_check()); cs.append(sparse_check())
    fd, fs = cd[-1][1], cs[-1][1]
    tcd, tcs = min(x[0] for x in cd), min(x[0] for x in cs)
    rec = {"n": n, "bw": bw, "nnz": nnz,
           "solve_dense_s": d[0], "solve_dense_copy_s": d[1], "solve_sparse_s": s[0], "solve_sparse_copy_s": s[1],
           "csr_build_both_s": min(tc), "check_dense_s": tcd, "check_sparse_s": tcs,
           "res_max_dense": float(fd[2]), "res_max_sparse": float(fs[2]), "orth_dense": float(fd[3]),
           "orth_sparse": float(fs[3]), "ipr_max_diff": float(np.abs(ipr_d - ipr_s).max())}
    lines.append("N = %d, half bandwidth %d, %d triplets per matrix, generalized, all columns, best of %d" % (n, bw, nnz, reps))
    rec["dense_host_matrices_s"] = t_form
    rec["dense_host_bytes"] = 4 * 8 * n * n           # A, B and the copies the call overwrites
    lines.append("  solve   dense ek_hip_solve        %8.4f s  (EK_STAGE_COPY %7.4f s); not counted: %.3f s to form the two "
                 "dense host matrices" % (d[0], d[1], t_form))
    lines.append("          ek_hip_solve_sparse       %8.4f s  (EK_STAGE_COPY %7.4f s, of it CSR build of A and B %7.4f s)"
                 % (s[0], s[1], min(tc)))
    lines.append("          sparse / dense            %8.3f     w and Z bit-identical" % (s[0] / d[0]))
    lines.append("  check   three ek_hip_check calls  %8.4f s" % tcd)
    lines.append("          ek_hip_check_sparse       %8.4f s" % tcs)
    lines.append("          sparse / dense            %8.3f     res_max %.2e / %.2e, orthogonality %.2e / %.2e, max |d ipr| %.1e"
                 % (tcs / tcd, fs[2], fd[2], fs[3], fd[3], rec["ipr_max_diff"]))
    lines.append("  json    " + json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--bw", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_timing.txt"))
    ap.add_argument("--host-files", default=None, help="directory for band_<N>_{A,B}.mtx")
    a = ap.parse_args()
    rc = solver.load_library().ek_hip_init(0)
    if rc:
        raise SystemExit("ek_hip_init failed: %d" % rc)
    lines = []
    for n in (int(x) for x in a.sizes.split(",")):
        run(n, a.bw, a.reps, lines, a.host_files)
        print("\n".join(lines[-8:]), flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
